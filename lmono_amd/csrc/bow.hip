// bow.hip -- LoopDetector::detectLoop's database on the device (mono_lidar_mapping/src/loop_detection/LoopDetector.cc:167-260 over DBoW2's
// TemplatedVocabulary::transform, BowVector and TemplatedDatabase::queryL1): DESIGN.md 6h holds the written definition these kernels and
// tests/bow_ref.py implement, for TF_IDF weighting and L1_NORM scoring.  Every fp64 sum is sequential in the order of 6h (the library is
// built with -ffp-contract=off), so the kernels and the restatement agree bit for bit.
//   k_bow_words    the descent of every pending descriptor: a thread per descriptor, a strict < scan over the (contiguous) children
//   k_bow_vector   a workgroup per pending keyframe: word ids bitonic-sorted in LDS (padded with 0x7fffffff), run heads compacted in
//                  order, a word's value by repeated addition, the norm by one thread's sequential sum, the division
//   k_bow_score    a thread per admitted entry: merge join of the query's row and the entry's row, the sum in ascending word id
//   k_bow_top      a workgroup per query: max_results rounds of "the least (s, id) after the last one taken"
// Every kernel body is a function of (job, block, thread) in plain C++, split at its barriers; the kernels below call the pieces with
// __syncthreads() between them, and lmono_amd/host/bow_test.cpp drives the same pieces with loops, without a GPU.  Every index that
// comes from data (a child range, a word id, a row length) is checked against the limits in the job before it is used.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BOW_HD __host__ __device__ __forceinline__
#else
#define BOW_HD inline
#endif

namespace lmono {

constexpr int kBowT = 256;             // threads of k_bow_words, k_bow_vector, k_bow_top
constexpr int kBowScoreT = 64;         // threads of k_bow_score (one entry each: small workgroups spread the entries over the CUs)
constexpr int kBowMaxKp = 16384;       // corners of a keyframe the LDS sort holds (64 KiB of int32)
constexpr int kBowMaxResults = 16;
constexpr int kBowPad = 0x7fffffff;    // sorts behind every word id
constexpr double kBowAlpha = 0.05, kBowBeta = 0.015;        // LoopDetector.cc:205, :210 -- constants of the reference, not parameters

// the tree, re-indexed at create time: node 0 is the root, the children of a node are child_begin .. child_begin + child_count - 1 in file order
struct BowVoc {
    const uint32_t *desc;                // [n_nodes][8]
    const int *child_begin, *child_count, *word;        // [n_nodes]; word: the leaf's word id, -1 for an inner node
    const double *weight;                // [n_words]
    int n_nodes, n_words, k, L;          // n_nodes counts the root
};

struct BowWordsJob {
    const uint32_t *desc;                // [n][8]
    int n;
    int *word;                           // [n]: word id, -1 where the descent ended outside the tables
    double *weight;                      // [n] or null
};

struct BowVecJob {
    int n;                               // descriptors of the keyframe
    int *word;                           // in: [n] word ids of k_bow_words; out: the vector's word ids, ascending
    double *val;                         // out: [<= n] values
    int *n_out;
};

struct BowResult { double score[kBowMaxResults]; int id[kBowMaxResults]; int n, pad; };

struct BowQueryJob {
    const int *bow_word;                 // [n_kf][max_kp]
    const double *bow_val;
    const int *bow_n;                    // [n_kf]
    int max_kp, n_kf, cur, max_id, max_results;
    double *s;                           // [>= cur] score sums of the entries
    int *flag;                           // [>= cur] 1: admitted and shares a word with the query
    BowResult *out;
};

BOW_HD int bow_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}

BOW_HD int bow_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// transform (TemplatedVocabulary.h:1217-1258)
BOW_HD void bow_words_body(const BowVoc &v, const BowWordsJob &j, int block, int tid)
{
    const size_t i = (size_t)block * kBowT + (size_t)tid;
    if (j.n <= 0 || i >= (size_t)j.n || v.n_nodes <= 0) return;
    uint32_t d[8];
    for (int q = 0; q < 8; q++) d[q] = j.desc[i * 8 + q];
    const size_t n_nodes = (size_t)v.n_nodes;
    size_t node = 0;
    for (int lv = 0; lv < v.L && v.child_count[node] > 0; ++lv) {
        const int cb = v.child_begin[node], cc = v.child_count[node] < v.k ? v.child_count[node] : v.k;
        if (cb <= 0) break;                                     // no node has the root as a child
        int best = 257;
        size_t at = node;
        for (int c = 0; c < cc; c++) {
            const size_t ch = (size_t)cb + (size_t)c;
            if (ch >= n_nodes) break;
            const uint32_t *cd = v.desc + ch * 8;
            int dist = 0;
            for (int q = 0; q < 8; q++) dist += bow_popc(d[q] ^ cd[q]);
            if (dist < best) { best = dist; at = ch; }          // strict <: the first of equal children
        }
        if (at == node) break;
        node = at;
    }
    int w = v.word[node];
    if (w < 0 || w >= v.n_words) w = -1;
    j.word[i] = w;
    if (j.weight) j.weight[i] = w >= 0 ? v.weight[(size_t)w] : 0.0;
}

// ---- k_bow_vector, piece by piece (s: P ints, P = bow_pow2(n); nt: threads)
BOW_HD void bow_vec_load(const BowVoc &v, const BowVecJob &j, int P, int *s, int tid, int nt)
{
    for (int i = tid; i < P; i += nt) {
        int w = kBowPad;
        if (i < j.n) {
            const int r = j.word[i];
            if (r >= 0 && r < v.n_words && v.weight[(size_t)r] > 0.0) w = r;          // a stop word (weight not > 0) is dropped
        }
        s[i] = w;
    }
}

BOW_HD void bow_vec_sort_step(int *s, int P, int k, int jj, int tid, int nt)
{
    for (int i = tid; i < P; i += nt) {
        const int l = i ^ jj;
        if (l <= i || l >= P) continue;
        const int a = s[i], b = s[l];
        const bool up = (i & k) == 0;
        if (up ? a > b : a < b) { s[i] = b; s[l] = a; }
    }
}

BOW_HD bool bow_vec_head(const int *s, int i) { return s[i] != kBowPad && (i == 0 || s[i] != s[i - 1]); }

// run heads in this thread's share [tid * per, (tid + 1) * per) of the sorted array
BOW_HD int bow_vec_count(const int *s, int P, int tid, int nt)
{
    const int per = (P + nt - 1) / nt, i0 = tid * per, i1 = i0 + per < P ? i0 + per : P;
    int n = 0;
    for (int i = i0; i < i1; i++) n += bow_vec_head(s, i) ? 1 : 0;
    return n;
}

// the heads of this thread's share go to word / val from `base` on: the value of a word is its weight added to itself once per occurrence
BOW_HD void bow_vec_emit(const BowVoc &v, const BowVecJob &j, const int *s, int P, int tid, int nt, int base)
{
    const int per = (P + nt - 1) / nt, i0 = tid * per, i1 = i0 + per < P ? i0 + per : P;
    for (int i = i0; i < i1; i++) {
        if (!bow_vec_head(s, i)) continue;
        const int w = s[i];
        if (w < 0 || w >= v.n_words || base < 0 || base >= j.n) return;
        const double wt = v.weight[(size_t)w];
        double val = wt;
        for (int r = i + 1; r < P && s[r] == w; r++) val = val + wt;
        j.word[base] = w; j.val[base] = val;
        base++;
    }
}

BOW_HD double bow_vec_norm(const BowVecJob &j, int m)
{
    double norm = 0.0;
    for (int i = 0; i < m; i++) norm = norm + j.val[i];
    return norm;
}

BOW_HD void bow_vec_divide(const BowVecJob &j, int m, double norm, int tid, int nt)
{
    if (!(norm > 0.0)) return;
    for (int i = tid; i < m; i += nt) j.val[i] = j.val[i] / norm;
}

// ---- queryL1 (TemplatedDatabase.h:656-723)
BOW_HD bool bow_admitted(int e, int cur, int max_id) { return e >= 0 && e < cur && (e < max_id || max_id == -1 || e == cur - 1); }

BOW_HD int bow_row_len(const BowQueryJob &j, size_t row)
{
    const int n = j.bow_n[row];
    return n < 0 ? 0 : (n > j.max_kp ? j.max_kp : n);
}

BOW_HD void bow_score_body(const BowQueryJob &j, int block, int tid, int nt)
{
    const size_t e = (size_t)block * (size_t)nt + (size_t)tid;
    if (j.cur < 0 || j.cur >= j.n_kf || e >= (size_t)j.cur) return;
    double sum = 0.0;
    int common = 0;
    if (bow_admitted((int)e, j.cur, j.max_id)) {
        const size_t per = (size_t)j.max_kp, qr = (size_t)j.cur;
        const int nq = bow_row_len(j, qr), nd = bow_row_len(j, e);
        const int *qw = j.bow_word + qr * per, *dw = j.bow_word + e * per;
        const double *qv = j.bow_val + qr * per, *dv = j.bow_val + e * per;
        int a = 0, b = 0;
        while (a < nq && b < nd) {
            const int wa = qw[a], wb = dw[b];
            if (wa == wb) {
                const double q = qv[a], d = dv[b];
                const double t = (fabs(q - d) - fabs(q)) - fabs(d);
                sum = common ? sum + t : t;
                common = 1;
                a++; b++;
            } else if (wa < wb) a++;
            else b++;
        }
    }
    j.s[e] = sum; j.flag[e] = common;
}

// the total order of the results: s ascending, ties to the lower entry
BOW_HD bool bow_less(double sa, int ia, double sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

// this thread's least flagged entry (e = tid, tid + nt, ...) that comes after (last_s, last_i); bi = -1: none
BOW_HD void bow_top_scan(const BowQueryJob &j, int tid, int nt, bool have_last, double last_s, int last_i, double &bs, int &bi)
{
    bs = 0.0; bi = -1;
    if (j.cur < 0 || j.cur >= j.n_kf) return;
    for (int e = tid; e < j.cur; e += nt) {
        if (!j.flag[e]) continue;
        const double s = j.s[e];
        if (have_last && !bow_less(last_s, last_i, s, e)) continue;
        if (bi < 0 || bow_less(s, e, bs, bi)) { bs = s; bi = e; }
    }
}

BOW_HD void bow_top_merge(double &as, int &ai, double bs, int bi)
{
    if (bi >= 0 && (ai < 0 || bow_less(bs, bi, as, ai))) { as = bs; ai = bi; }
}

BOW_HD int bow_top_limit(const BowQueryJob &j) { return j.max_results < 0 ? 0 : (j.max_results > kBowMaxResults ? kBowMaxResults : j.max_results); }

// LoopDetector::detectLoop's rule over the (at most 4) results of query(cur, 4, cur - gap) (LoopDetector.cc:200-259, without DEBUG_IMAGE)
inline int bow_detect_rule(int cur, int gap, int n, const int *id, const double *score)
{
    if (cur - gap < 0) return -1;
    bool find_loop = false;
    if (n >= 1 && score[0] > kBowAlpha)
        for (int i = 1; i < n; i++) if (score[i] > kBowBeta) find_loop = true;
    if (!(find_loop && cur > 5)) return -1;
    int min_index = -1;
    for (int i = 0; i < n; i++)
        if (min_index == -1 || (id[i] < min_index && score[i] > kBowBeta)) min_index = id[i];          // i = 0 always seeds min_index
    return min_index;
}

// ---- the vocabulary on the host: the checks of DESIGN.md 6h and the re-indexing (loadBin, TemplatedVocabulary.h:1529-1538)
struct BowVocHost {
    int k = 0, L = 0, n_nodes = 0, n_words = 0;          // n_nodes counts the root
    std::vector<uint32_t> desc;
    std::vector<int> child_begin, child_count, word;
    std::vector<double> weight;
    BowVoc view() const { return BowVoc{ desc.data(), child_begin.data(), child_count.data(), word.data(), weight.data(), n_nodes, n_words, k, L }; }
};

// null when the vocabulary is well formed (out is filled), else the reason.  The same checks, in this order and in these words, are
// lmono_amd.capi.check_brief_vocabulary's
inline const char *bow_voc_build(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *node_id, const int32_t *parent_id, const double *weight,
                                 const uint32_t *desc, int n_words, const int32_t *word_node_id, const int32_t *word_id, BowVocHost &out)
{
    if (k < 2 || k > 64) return "brief vocabulary: k outside 2..64";
    if (L < 1 || L > 10) return "brief vocabulary: L outside 1..10";
    if (scoring != 0 || weighting != 0) return "brief vocabulary: only L1_NORM scoring (0) with TF_IDF weighting (0) is built";
    if (n_nodes < 1 || n_nodes > 16777215) return "brief vocabulary: nNodes outside 1..16777215";
    if (n_words < 1 || n_words > n_nodes) return "brief vocabulary: nWords outside 1..nNodes";
    if (!node_id || !parent_id || !weight || !desc || !word_node_id || !word_id) return "brief vocabulary: a null array";
    const size_t n = (size_t)n_nodes, total = n + 1;
    std::vector<int> rec(total, -1);                     // file record of node id
    for (size_t r = 0; r < n; r++) {
        const int32_t id = node_id[r];
        if (id < 1 || id > n_nodes || rec[(size_t)id] != -1) return "brief vocabulary: nodeIds are not exactly 1..nNodes, each once";
        rec[(size_t)id] = (int)r;
    }
    for (size_t r = 0; r < n; r++)
        if (parent_id[r] < 0 || parent_id[r] > n_nodes || parent_id[r] == node_id[r]) return "brief vocabulary: a parentId outside 0..nNodes or equal to its own nodeId";
    for (size_t r = 0; r < n; r++)
        if (!(weight[r] >= 0.0) || !std::isfinite(weight[r])) return "brief vocabulary: a weight that is negative or not finite";
    // children of every node id in file order: counting sort by parent (stable)
    std::vector<int> cnt(total + 1, 0), kids(n);
    for (size_t r = 0; r < n; r++) cnt[(size_t)parent_id[r] + 1]++;
    for (size_t p = 0; p < total; p++) {
        if (cnt[p + 1] > k) return "brief vocabulary: an inner node with more than k children";
        cnt[p + 1] += cnt[p];
    }
    {
        std::vector<int> at(cnt.begin(), cnt.end() - 1);
        for (size_t r = 0; r < n; r++) kids[(size_t)at[(size_t)parent_id[r]]++] = node_id[r];
    }
    // breadth first from the root: new index = position in the visit order, so the children of a node are contiguous
    std::vector<int> order, depth(total, 0), new_of(total, -1);
    order.reserve(total);
    order.push_back(0); new_of[0] = 0;
    for (size_t h = 0; h < order.size(); h++) {
        const size_t id = (size_t)order[h];
        for (int c = cnt[id]; c < cnt[id + 1]; c++) {
            const size_t ch = (size_t)kids[(size_t)c];
            if (new_of[ch] != -1 || depth[id] + 1 > L) return "brief vocabulary: a node unreachable from the root, or deeper than L";
            depth[ch] = depth[id] + 1;
            new_of[ch] = (int)order.size();
            order.push_back((int)ch);
        }
    }
    if (order.size() != total) return "brief vocabulary: a node unreachable from the root, or deeper than L";
    out.k = k; out.L = L; out.n_nodes = (int)total; out.n_words = n_words;
    out.desc.assign(total * 8, 0u); out.child_begin.assign(total, 0); out.child_count.assign(total, 0); out.word.assign(total, -1); out.weight.assign((size_t)n_words, 0.0);
    size_t leaves = 0;
    for (size_t h = 0; h < total; h++) {
        const size_t id = (size_t)order[h];
        out.child_count[h] = cnt[id + 1] - cnt[id];
        out.child_begin[h] = out.child_count[h] > 0 ? new_of[(size_t)kids[(size_t)cnt[id]]] : 0;
        if (out.child_count[h] == 0) leaves++;
        if (id > 0) for (int q = 0; q < 8; q++) out.desc[h * 8 + (size_t)q] = desc[(size_t)rec[id] * 8 + (size_t)q];
    }
    const char *bad_words = "brief vocabulary: the words are not a bijection between 0..nWords-1 and the leaves";
    if (leaves != (size_t)n_words) return bad_words;
    std::vector<char> seen((size_t)n_words, 0);
    for (int w = 0; w < n_words; w++) {
        const int32_t id = word_node_id[w], wid = word_id[w];
        if (id < 1 || id > n_nodes || wid < 0 || wid >= n_words || seen[(size_t)wid]) return bad_words;
        const size_t h = (size_t)new_of[(size_t)id];
        if (out.child_count[h] != 0 || out.word[h] != -1) return bad_words;
        seen[(size_t)wid] = 1;
        out.word[h] = wid;
        out.weight[(size_t)wid] = weight[(size_t)rec[(size_t)id]];
    }
    return nullptr;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(kBowT) void k_bow_words(BowVoc v, const BowWordsJob *jobs)
{
    bow_words_body(v, jobs[blockIdx.x], (int)blockIdx.y, (int)threadIdx.x);        // grid (jobs, blocks of a job)
}

// dynamic LDS: lds_ints ints (a power of two that holds the largest job)
__global__ __launch_bounds__(kBowT) void k_bow_vector(BowVoc v, const BowVecJob *jobs, int lds_ints)
{
    extern __shared__ int s_bow[];
    __shared__ int s_cnt[kBowT];
    __shared__ double s_norm;
    BowVecJob j = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    if (j.n < 0) j.n = 0;
    const int P = bow_pow2(j.n);
    if (P > lds_ints) return;                                   // uniform: the host sized the LDS for the largest job
    bow_vec_load(v, j, P, s_bow, tid, kBowT);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            bow_vec_sort_step(s_bow, P, k, jj, tid, kBowT);
            __syncthreads();
        }
    s_cnt[tid] = bow_vec_count(s_bow, P, tid, kBowT);
    __syncthreads();
    int base = 0, m = 0;
    for (int t = 0; t < kBowT; t++) { const int c = s_cnt[t]; m += c; base += t < tid ? c : 0; }
    bow_vec_emit(v, j, s_bow, P, tid, kBowT, base);
    __syncthreads();
    if (m > j.n) m = j.n;
    if (tid == 0) { s_norm = bow_vec_norm(j, m); *j.n_out = m; }
    __syncthreads();
    bow_vec_divide(j, m, s_norm, tid, kBowT);
}

__global__ __launch_bounds__(kBowScoreT) void k_bow_score(const BowQueryJob *jobs)
{
    bow_score_body(jobs[blockIdx.y], (int)blockIdx.x, (int)threadIdx.x, kBowScoreT);
}

__global__ __launch_bounds__(kBowT) void k_bow_top(const BowQueryJob *jobs)
{
    __shared__ double s_s[kBowT];
    __shared__ int s_i[kBowT];
    const BowQueryJob &j = jobs[blockIdx.x];
    const int tid = (int)threadIdx.x, limit = bow_top_limit(j);
    bool have_last = false;
    double last_s = 0.0;
    int last_i = -1, n = 0;
    for (int r = 0; r < limit; r++) {
        double bs; int bi;
        bow_top_scan(j, tid, kBowT, have_last, last_s, last_i, bs, bi);
        s_s[tid] = bs; s_i[tid] = bi;
        __syncthreads();
        for (int stride = kBowT / 2; stride > 0; stride >>= 1) {
            if (tid < stride) bow_top_merge(s_s[tid], s_i[tid], s_s[tid + stride], s_i[tid + stride]);
            __syncthreads();
        }
        last_s = s_s[0]; last_i = s_i[0];
        __syncthreads();
        if (last_i < 0) break;                                  // uniform
        have_last = true;
        if (tid == 0) { j.out->id[r] = last_i; j.out->score[r] = -last_s / 2.0; }
        n++;
    }
    if (tid == 0) { j.out->n = n; j.out->pad = 0; }
}

#endif // __HIPCC__

} // namespace lmono
