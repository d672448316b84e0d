// sacia.hpp -- the arithmetic of the sample-consensus initial alignment on FPFH descriptors: the
// pcl::SampleConsensusInitialAlignment of MapBuilder::alignmentToMap (computeInitialAlignment: min_sample_dist 0.5, max_correspondence_dist 1.0,
// nr_iters 30), the coarse map-to-map alignment the reference carries commented out (mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210).
// One text for the kernels (sacia.hip), for a CPU program (host/sacia_test.cpp) and for the host side of the C ABI; every float operation is a
// single IEEE operation (build with -ffp-contract=off).  The definition is this project's own.  Parity with PCL is unpinned.
//
// Inputs: source and target keypoints [m][3] float32 with descriptors [m][33] float32 and flags (fpfh.hpp).  A keypoint is usable iff its flag is 1;
// the usable ones of a side, in keypoint order, are its list: ns source and nt target entries, both >= 3 (else refused).  The centres cs, ct are the
// first entries of the lists; u = s - cs and w = t - ct per axis in float32, every |u_a|, |w_a| < 2048 (else refused): icp_fix is exact on them.
// Candidates of source entry i: the K = min(k_corr, nt) target entries of smallest descriptor distance
//   D(i, j) = the 33 terms (a_b - b_b) * (a_b - b_b) in float32, added in index order from 0.0f,
// ordered by (D, j): ties go to the lowest target index.  Descriptors are finite values of 0 .. 100, so every distance is finite.
// Hypothesis h: key = pnp_key(seed, kSaciaKey, h), draw d is pnp_mix(key ^ d), an index below n is (r * n) >> 32 (the PnP RANSAC's generator).
//   Sample: draws d = 0, 1, ... pick source entries; a draw is taken iff it differs from every entry taken so far and its float32 sor_d2 to each
//   of them is >= min_sample_dist * min_sample_dist.  Three taken within kSaciaMaxDraws draws, else the hypothesis is void.
//   Partners: entry e (0, 1, 2) of the sample takes candidate (pnp_mix(key ^ (kSaciaMaxDraws + e)) * K) >> 32 of its source entry.
//   Fit: icp_terms of the three (u, w) pairs added into one IcpSums, icp_solve: w ~ R u + tau, the aligner's closed form.
//   Error: for every source entry, q = icp_q_axis(R row, tau, ct, u) per axis, d2 = the least sor_d2(q, t) over the target entries (a minimum:
//   order-free), truncated at mc2 = max_corr * max_corr (float32), as (uint64)((double)d2 * 2^24), summed as integers; d2 <= mc2 is an inlier.
// Best: the least (error, h) over the hypotheses that are not void.  Transform: [R | ((double)ct + tau) - R cs], row-major 3 x 4 fp64, the layout of
// lmono_icp_transform and lmono_icp_set_guess.
#pragma once
#include "fpfh.hpp"
#if defined(__HIPCC__)
#include "pnp.hip"
#else
#include <cstdint>
#endif

namespace lmono {

#if !defined(__HIPCC__)
// the generator of pnp.hip, restated for the host program (the values are those of pnp_mix / pnp_key)
inline uint32_t pnp_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
inline uint32_t pnp_key(uint32_t seed, uint32_t key, uint32_t h) { return pnp_mix(pnp_mix(pnp_mix(seed ^ 0x9e3779b9u) ^ key) ^ h); }
#endif

constexpr int kSaciaMaxK = 32;                  // k_corr
constexpr int kSaciaMaxHyp = 65536;
constexpr int kSaciaMaxDraws = 64;              // draws of one sample before the hypothesis is void
constexpr uint32_t kSaciaKey = 0x5ac1au;        // the `key` of pnp_key for this stage
constexpr float kSaciaMaxCorr = 16.0f;
constexpr unsigned long long kSaciaVoid = ~0ull;   // the error word of a void hypothesis

// the error words: d2 <= 16 * 16 = 2^8, so a term is at most 2^32 and 4096 of them stay below 2^44
static_assert(kSaciaMaxCorr * kSaciaMaxCorr <= 256.0f && kFpfhMaxKeypoints <= 4096, "an error sum stays below 2^44");
static_assert(kSaciaMaxDraws + 3 <= 256, "the draws of a hypothesis are distinct small integers");

LMONO_VM_HD bool sacia_params_ok(float min_sample_dist, float max_corr, int k_corr, int n_hyp)
{
    return min_sample_dist >= 0.0f && min_sample_dist <= 4096.0f && max_corr > 0.0f && max_corr <= kSaciaMaxCorr && k_corr >= 1 && k_corr <= kSaciaMaxK &&
           n_hyp >= 1 && n_hyp <= kSaciaMaxHyp;
}

LMONO_VM_HD int sacia_below(uint32_t r, int n) { return (int)(((uint64_t)r * (uint64_t)(uint32_t)n) >> 32); }

// the squared descriptor distance
LMONO_VM_HD float sacia_desc_d2(const float *a, const float *b)
{
    float s = 0.0f;
    for (int k = 0; k < kFpfhDim; k++) { const float d = a[k] - b[k]; s = s + d * d; }
    return s;
}

// (d, j) before (bd, bj)
LMONO_VM_HD bool sacia_before(float d, int j, float bd, int bj) { return d < bd || (d == bd && j < bj); }

// The sample of hypothesis `key` among ns source entries at u (centred, [ns][3]): three entries, false: void
LMONO_VM_HD bool sacia_sample(uint32_t key, int ns, const float *u, float msd2, int idx[3])
{
    int have = 0;
    for (int d = 0; d < kSaciaMaxDraws && have < 3; d++) {
        const int c = sacia_below(pnp_mix(key ^ (uint32_t)d), ns);
        bool ok = true;
        for (int q = 0; q < 3; q++)
            if (q < have) {
                const int e = idx[q];
                ok = ok && e != c && sor_d2(u[3 * e], u[3 * e + 1], u[3 * e + 2], u[3 * c], u[3 * c + 1], u[3 * c + 2]) >= msd2;
            }
        if (ok) {                                   // idx[have] = c under static indices
            if (have == 0) idx[0] = c; else if (have == 1) idx[1] = c; else idx[2] = c;
            have++;
        }
    }
    return have == 3;
}

// The fit of hypothesis `key`: false: void.  cand: [ns][K] target entries; u [ns][3], w [nt][3] centred
LMONO_VM_HD bool sacia_fit(uint32_t key, int ns, const float *u, const float *w, const int *cand, int K, float msd2, double *R, double *tau)
{
    int idx[3] = { 0, 0, 0 };
    if (!sacia_sample(key, ns, u, msd2, idx)) return false;
    IcpSums s;
    s.N = 0; s.E = 0;
    for (int a = 0; a < 3; a++) { s.Su[a] = 0; s.Sw[a] = 0; }
    for (int e = 0; e < 9; e++) { s.hi[e] = 0; s.lo[e] = 0; }
    for (int e = 0; e < 3; e++) {
        const int i = e == 0 ? idx[0] : (e == 1 ? idx[1] : idx[2]);
        const int j = cand[(size_t)i * K + sacia_below(pnp_mix(key ^ (uint32_t)(kSaciaMaxDraws + e)), K)];
        IcpSums t;
        icp_terms(u + 3 * i, w + 3 * j, 0.0f, t);
        s.N += t.N;
        for (int a = 0; a < 3; a++) { s.Su[a] += t.Su[a]; s.Sw[a] += t.Sw[a]; }
        for (int k = 0; k < 9; k++) { s.hi[k] += t.hi[k]; s.lo[k] += t.lo[k]; }
    }
    icp_solve(s, R, tau);
    return true;
}

// one term of the error: the least squared distance, truncated
LMONO_VM_HD unsigned long long sacia_term(float d2, float mc2) { return (unsigned long long)((double)(d2 <= mc2 ? d2 : mc2) * 16777216.0); }

// the transform of a fit
LMONO_VM_HD void sacia_transform(const double *R, const double *tau, const float cs[3], const float ct[3], double *T)
{
    for (int a = 0; a < 3; a++) {
        const double *r = R + 3 * a;
        for (int b = 0; b < 3; b++) T[4 * a + b] = r[b];
        T[4 * a + 3] = ((double)ct[a] + tau[a]) - ((r[0] * (double)cs[0] + r[1] * (double)cs[1]) + r[2] * (double)cs[2]);
    }
}

} // namespace lmono
