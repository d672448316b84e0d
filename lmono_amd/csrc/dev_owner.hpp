// dev_owner.hpp -- the one owner of the device and pinned host memory behind a C ABI handle (or of one call's temporaries).
// Whatever it allocated and has not released is freed when it goes, so a create function is a && chain of alloc() calls whose
// failure path is "destroy the handle", and a destroy function frees nothing by hand.
//
// A buffer that has become too small grows by one of two policies; the call site names the one it chose:
//   grow_replace  the new buffer is allocated, then the old one is freed (hipFree waits for the device).  For handles whose every call
//                 ends synchronised, so that nothing in flight reads the old buffer.
//   grow_keep     the outgrown buffer stays owned until the owner goes: kernels or copies in flight may still read it.
// Both size alike: the capacity doubles from max(cap, floor) until it holds what is needed.
//
// With LMONO_DEV_OWNER_TEST defined the HIP runtime is not included: the including file declares hipMalloc, hipFree, hipHostMalloc,
// hipHostFree, hipMemset, hipMemcpy and their enums itself (dev_owner_test.cpp, a host program over malloc).
#pragma once
#ifndef LMONO_DEV_OWNER_TEST
#include <hip/hip_runtime.h>
#endif
#include <algorithm>
#include <cstddef>
#include <vector>

struct DevOwner {
    DevOwner() = default;
    DevOwner(const DevOwner &) = delete;
    DevOwner &operator=(const DevOwner &) = delete;
    ~DevOwner() { clear(); }
    // free everything now (a destroy function that has more to take down behind the memory)
    void clear()
    {
        for (void *q : dev_) (void)hipFree(q);
        for (void *q : host_) (void)hipHostFree(q);
        dev_.clear(); host_.clear();
    }

    // count elements of device memory (a count of 0 is allocated as 1); on failure p is untouched and nothing is recorded
    template <typename T> bool alloc(T *&p, size_t count)
    {
        void *q = nullptr;
        if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
        dev_.push_back(q);
        p = (T *)q;
        return true;
    }
    // ... zeroed.  A failed memset returns false with the buffer owned (p untouched): it goes with the owner
    template <typename T> bool alloc_zero(T *&p, size_t count)
    {
        T *q = nullptr;
        if (!alloc(q, count) || hipMemset(q, 0, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
        p = q;
        return true;
    }
    // ... holding a copy of src
    template <typename T> bool upload(const T *&p, const std::vector<T> &src)
    {
        T *q = nullptr;
        if (!alloc(q, src.size()) || (!src.empty() && hipMemcpy(q, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)) return false;
        p = q;
        return true;
    }
    // count elements of pinned host memory
    template <typename T> bool pinned(T *&p, size_t count)
    {
        void *q = nullptr;
        if (hipHostMalloc(&q, (count ? count : 1) * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
        host_.push_back(q);
        p = (T *)q;
        return true;
    }
    // free one buffer now and null p; a p this owner does not hold (null, or released before through another variable) is only nulled
    template <typename T> void release(T *&p)
    {
        void *q = (void *)p;
        p = nullptr;
        auto it = std::find(dev_.begin(), dev_.end(), q);
        if (it != dev_.end()) { (void)hipFree(q); dev_.erase(it); return; }
        it = std::find(host_.begin(), host_.end(), q);
        if (it != host_.end()) { (void)hipHostFree(q); host_.erase(it); }
    }

    static size_t grown(size_t cap, size_t need, size_t floor)
    {
        size_t nc = std::max(cap, std::max<size_t>(floor, 1));
        while (nc < need) nc <<= 1;
        return nc;
    }
    // p holds cap * per elements; make cap >= need.  If the allocation fails, the old buffer and cap stand.
    template <typename T, typename C> bool grow_replace(T *&p, C &cap, size_t need, size_t floor, size_t per = 1)
    {
        if (need <= (size_t)cap) return true;
        const size_t nc = grown((size_t)cap, need, floor);
        T *q = nullptr;
        if (!alloc(q, nc * per)) return false;
        release(p);
        p = q; cap = (C)nc;
        return true;
    }
    template <typename T, typename C> bool grow_keep(T *&p, C &cap, size_t need, size_t floor)
    {
        if (need <= (size_t)cap) return true;
        const size_t nc = grown((size_t)cap, need, floor);
        if (!alloc(p, nc)) return false;
        cap = (C)nc;
        return true;
    }
    template <typename T, typename C> bool grow_keep_pinned(T *&p, C &cap, size_t need, size_t floor)
    {
        if (need <= (size_t)cap) return true;
        const size_t nc = grown((size_t)cap, need, floor);
        if (!pinned(p, nc)) return false;
        cap = (C)nc;
        return true;
    }

private:
    std::vector<void *> dev_, host_;
};

// "job array + k result ints per stream" of a batched call, owned by the call's first handle: at least n jobs, doubling from 1.
// grow_replace: every batched entry point ends synchronised, so no launch reads the outgrown table
template <typename J, typename C> static bool job_table(DevOwner &mem, J *&jobs, int *&results, C &cap, int n, int k)
{
    C cj = cap, cr = cap;       // cap moves only when both halves have grown
    if (!mem.grow_replace(jobs, cj, (size_t)n, /*floor=*/1) || !mem.grow_replace(results, cr, (size_t)n, /*floor=*/1, /*per=*/(size_t)k)) return false;
    cap = cj;
    return true;
}
