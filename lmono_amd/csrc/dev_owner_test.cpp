// dev_owner_test.cpp -- host check of dev_owner.hpp: the seven HIP calls it makes are defined here over malloc / free with a table of
// live blocks and a "fail the N-th call" switch.  Stand-alone (own main), built with the address and undefined-behaviour sanitizers by
// tests/test_dev_owner_cpu.py; exits non-zero at the first violated expectation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
constexpr unsigned hipHostMallocDefault = 0;

static std::map<void *, size_t> g_dev, g_host;      // live blocks and their sizes
static int g_calls = 0, g_fail_at = 0;              // the g_fail_at-th call from now fails (0: none)

static bool failing() { return g_fail_at && ++g_calls == g_fail_at; }
static void fail_call(int n) { g_calls = 0; g_fail_at = n; }

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static hipError_t hipMalloc(void **p, size_t bytes)
{
    if (failing()) return hipErrorOutOfMemory;
    EXPECT(bytes > 0);
    *p = std::malloc(bytes);
    std::memset(*p, 0xa5, bytes);
    g_dev[*p] = bytes;
    return hipSuccess;
}
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
    if (failing()) return hipErrorOutOfMemory;
    EXPECT(bytes > 0);
    *p = std::malloc(bytes);
    g_host[*p] = bytes;
    return hipSuccess;
}
static hipError_t hipFree(void *p) { EXPECT(g_dev.erase(p) == 1); std::free(p); return hipSuccess; }            // a double free or a foreign pointer ends the program
static hipError_t hipHostFree(void *p) { EXPECT(g_host.erase(p) == 1); std::free(p); return hipSuccess; }
static hipError_t hipMemset(void *p, int v, size_t bytes)
{
    if (failing()) return hipErrorInvalidValue;
    EXPECT(g_dev.count(p) && g_dev[p] >= bytes);
    std::memset(p, v, bytes);
    return hipSuccess;
}
static hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind)
{
    if (failing()) return hipErrorInvalidValue;
    EXPECT(g_dev.count(dst) && g_dev[dst] >= bytes);
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}

#define LMONO_DEV_OWNER_TEST
#include "dev_owner.hpp"

static void nothing_live() { EXPECT(g_dev.empty() && g_host.empty()); }

static void test_alloc()
{
    {
        DevOwner m;
        double *p = nullptr;
        EXPECT(m.alloc(p, 0) && p && g_dev.at(p) == sizeof(double));        // a count of 0 is one element
        p[0] = 1.0;
        int *q = nullptr, *const q0 = q;
        const auto live = g_dev;
        fail_call(1);
        EXPECT(!m.alloc(q, 16) && q == q0 && g_dev == live);                 // a failure leaves p and the live table as they were
        fail_call(0);
        float *a = nullptr, *b = nullptr; char *h = nullptr;
        EXPECT(m.alloc(a, 3) && m.alloc(b, 5) && m.pinned(h, 7));
        EXPECT(g_dev.size() == 3 && g_host.size() == 1 && g_host.at(h) == 7);
    }
    nothing_live();                                                          // after a run of successes
    {
        DevOwner m;
        int *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr; char *h = nullptr;
        fail_call(3);
        const bool ok = m.alloc(a, 4) && m.pinned(h, 8) && m.alloc(b, 4) && m.alloc(c, 4) && m.alloc(d, 4);        // the shape of every create function
        fail_call(0);
        EXPECT(!ok && a && h && !b && !c && !d && g_dev.size() == 1 && g_host.size() == 1);
    }
    nothing_live();                                                          // after a failure in the middle of the chain
}

static void test_release()
{
    DevOwner m;
    int *a = nullptr, *b = nullptr, *c = nullptr, *none = nullptr; char *h = nullptr;
    EXPECT(m.alloc(a, 1) && m.alloc(b, 1) && m.alloc(c, 1) && m.pinned(h, 1));
    int *b2 = b;
    m.release(b);                                                            // a middle element
    EXPECT(!b && g_dev.size() == 2 && g_dev.count(a) && g_dev.count(c));
    m.release(b2);                                                           // the same block through a second variable: found nowhere, nothing freed
    EXPECT(!b2 && g_dev.size() == 2);
    m.release(none);
    EXPECT(!none && g_dev.size() == 2 && g_host.size() == 1);
    m.release(h);
    EXPECT(!h && g_host.empty());
    a[0] = c[0] = 7;                                                         // the others are still there
}

template <bool kReplace> static void grow_steps(size_t floor, const size_t (&want)[3])
{
    {
        DevOwner m;
        int *p = nullptr; short *r = nullptr;
        int cap = 0, cap_r = 0;
        const size_t needs[3] = { 1, 3, 5 };
        size_t blocks = 0;
        for (int i = 0; i < 3; i++) {
            const int before = cap;
            if (kReplace) { EXPECT(m.grow_replace(p, cap, needs[i], floor) && m.grow_replace(r, cap_r, needs[i], floor, /*per=*/3)); }
            else EXPECT(m.grow_keep(p, cap, needs[i], floor));
            EXPECT((size_t)cap == want[i] && g_dev.at(p) == want[i] * sizeof(int));
            blocks += cap != before;
            if (kReplace) EXPECT(cap_r == cap && g_dev.at(r) == want[i] * 3 * sizeof(short) && g_dev.size() == 2);     // exactly one live block per array
            else EXPECT(g_dev.size() == blocks);                                                                   // the outgrown blocks stay live
            p[cap - 1] = i;
        }
        int *const p0 = p;
        const int cap0 = cap;
        const auto live = g_dev;
        fail_call(1);
        EXPECT(!(kReplace ? m.grow_replace(p, cap, (size_t)cap0 + 1, floor) : m.grow_keep(p, cap, (size_t)cap0 + 1, floor)));
        fail_call(0);
        EXPECT(p == p0 && cap == cap0 && g_dev == live);                     // a failed growth: the old pointer and cap stand ...
        p[cap - 1] = 9;                                                      // ... and are usable
    }
    nothing_live();
}

static void test_grow()
{
    grow_steps<true>(1, { 1, 4, 8 });
    grow_steps<true>(4, { 4, 4, 8 });
    grow_steps<false>(1, { 1, 4, 8 });
    grow_steps<false>(4, { 4, 4, 8 });
    {
        DevOwner m;
        double *p = nullptr; size_t cap = 0;
        int *h = nullptr; size_t cap_h = 0;
        EXPECT(m.grow_keep(p, cap, 10, /*floor=*/1024) && cap == 1024 && g_dev.at(p) == 1024 * sizeof(double));
        EXPECT(m.grow_keep(p, cap, 1024, 1024) && cap == 1024 && g_dev.size() == 1);
        EXPECT(m.grow_keep(p, cap, 1025, 1024) && cap == 2048 && g_dev.at(p) == 2048 * sizeof(double) && g_dev.size() == 2);
        EXPECT(m.grow_keep_pinned(h, cap_h, 1, 1024) && cap_h == 1024 && m.grow_keep_pinned(h, cap_h, 1025, 1024) && cap_h == 2048);
        EXPECT(g_host.size() == 2 && g_host.at(h) == 2048 * sizeof(int));
    }
    nothing_live();
    {   // the job table of a batched call: both halves at one capacity, which moves only when both have grown
        DevOwner m;
        long *jobs = nullptr; int *res = nullptr; int cap = 0;
        EXPECT(job_table(m, jobs, res, cap, 3, 2) && cap == 4 && g_dev.at(jobs) == 4 * sizeof(long) && g_dev.at(res) == 8 * sizeof(int) && g_dev.size() == 2);
        fail_call(2);
        EXPECT(!job_table(m, jobs, res, cap, 5, 2) && cap == 4 && g_dev.size() == 2 && g_dev.at(jobs) >= 4 * sizeof(long) && g_dev.at(res) == 8 * sizeof(int));
        fail_call(0);
        EXPECT(job_table(m, jobs, res, cap, 5, 2) && cap == 8 && g_dev.at(jobs) == 8 * sizeof(long) && g_dev.at(res) == 16 * sizeof(int) && g_dev.size() == 2);
        EXPECT(job_table(m, jobs, res, cap, 1, 2) && cap == 8 && g_dev.size() == 2);
    }
    nothing_live();
}

static void test_zero_and_upload()
{
    {
        DevOwner m;
        unsigned char *z = nullptr, *z0 = nullptr;
        EXPECT(m.alloc_zero(z, 33));
        for (int i = 0; i < 33; i++) EXPECT(z[i] == 0);                      // the mock's hipMalloc fills with 0xa5
        EXPECT(m.alloc_zero(z0, 0) && z0[0] == 0);
        int *w = nullptr;
        fail_call(2);                                                        // the memset
        EXPECT(!m.alloc_zero(w, 8) && !w && g_dev.size() == 3);              // false, the buffer owned ...
        fail_call(0);
        const std::vector<int> src = { 3, 1, 4, 1, 5 }, none;
        const int *u = nullptr, *e = nullptr;
        EXPECT(m.upload(u, src) && std::memcmp(u, src.data(), sizeof(int) * src.size()) == 0);
        EXPECT(m.upload(e, none) && e && g_dev.at((void *)e) == sizeof(int));
        fail_call(2);                                                        // the copy
        EXPECT(!m.upload(u, src));
        fail_call(0);
    }
    nothing_live();                                                          // ... so nothing leaks
}

int main()
{
    test_alloc();
    test_release();
    nothing_live();
    test_grow();
    test_zero_and_upload();
    std::puts("dev_owner ok");
    return 0;
}
