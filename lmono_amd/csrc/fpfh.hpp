// fpfh.hpp -- the arithmetic of the FPFH descriptors at keypoints: the pcl::FPFHEstimation with setSearchSurface and
// setRadiusSearch(0.05) of MapBuilder::alignmentToMap, the coarse map-to-map alignment the reference carries commented out
// (mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210).  One text for the kernels (fpfh.hip), for a CPU program (host/fpfh_test.cpp) and
// for the host side of the C ABI; every float operation is a single IEEE operation (build with -ffp-contract=off).  The definition is this
// project's own: a descriptor is a pure function of the SET of surface points with their normals and of the keypoint.  Parity with PCL is unpinned.
//
// Surface: a cloud with one record per point (normals.hpp).  Valid points, origin, span: the rules of a grid with an origin (cell_grid.hpp) at
// inv = 1.0f / h.  A point has a normal iff it is valid, in span and its record's nx is not NaN (a record is all NaN or has none).  Only
// points with a normal take part.  A keypoint is three finite floats, not necessarily a point of the surface; it is usable iff sor_cell accepts
// it at the same inv.  An unusable keypoint has no neighbours.
// Needed points: every point with a normal within r of some usable keypoint, sor_d2(keypoint, point) <= r * r in float32.  Only these get an SPFH,
// as in PCL.
// Pair features of the needed point i and a point j with a normal, 0 < sor_d2(p_i, p_j) <= r * r (so duplicates of p_i and i itself are no
// pairs): PCL's computePairFeatures in fp64 from the float32 coordinates and normals, without transcendentals (fpfh_pair):
//   dp = p_j - p_i per axis; f4 = sqrt((dp0 dp0 + dp1 dp1) + dp2 dp2); a1 = ((n_i . dp)) / f4, a2 = ((n_j . dp)) / f4, dots as (x + y) + z.
//   If |a1| < |a2| (PCL: acos|a1| > acos|a2|) the roles swap: n1 = n_j, n2 = n_i, dp = -dp, f3 = -a2; else n1 = n_i, n2 = n_j, f3 = a1.
//   v = dp x n1, vn = sqrt(v . v); vn == 0 skips the pair, as PCL does.  u = n1 x v.  f2 = (v . n2) / vn; x = n1 . n2, y = (u . n2) / vn.
// Bins, 11 per feature: f2 and f3 by floor((f + 1) * 5.5) clamped to 0 .. 10 (fpfh_bin); the angle of (x, y) by comparisons against the eleven
// edge directions -pi + 2 pi k / 11 written as fp64 literals (fpfh_angle_bin): no atan2, whose last place differs between libraries.
// SPFH of a needed point: 33 counts (angle | f2 | f3, FPFHSignature33's order) and the pair count n_i, integers below 2^26.
// FPFH of keypoint k: over every needed j with sor_d2(k, j) <= r * r and n_j > 0, the sums of W_j * count_j[b] with the integer weight
//   W_j = (uint64)(2^40 / ((double)max(d2, 2^-20) * (double)n_j))        (fpfh_weight; PCL: 1 / d2 times the SPFH's 100 / n_j),
// each product split into hi = P >> 32 and lo = P & (2^32 - 1) and summed as integers (fpfh_add): exact in any order.  The clamp of d2 at 2^-20 m^2
// makes a surface point AT the keypoint count with the largest weight; PCL skips it (a division by zero there).  That deviation is deliberate:
// a keypoint taken from the cloud keeps its own point's SPFH.  Then per sub-histogram v_b = (double)hi_b * 2^32 + (double)lo_b, total = the
// eleven v_b added in index order, out_b = (float)((v_b * 100.0) / total).  A keypoint with no contributing j gets 33 zeros, count 0 and flag 0.
//
// Why the grid cannot change the result: the argument at the head of sor.hpp, as for the normals: with sor_rho(R, h) >= r every point within r of a
// query lies in the cube of R rings about the query's cell; neighbours are selected by value and every sum is an integer.
#pragma once
#include "normals.hpp"

namespace lmono {

constexpr int kFpfhBins = 11, kFpfhDim = 33;
constexpr int kFpfhRow = kFpfhDim + 1;               // a stored SPFH: 33 counts and the pair count
constexpr int kFpfhMaxKeypoints = 4096;
constexpr float kFpfhMaxRadius = 4.0f;
constexpr long long kFpfhMaxPoints = 1ll << 26;
constexpr float kFpfhMinD2 = 9.5367431640625e-07f;  // 2^-20 m^2: the floor of d2 in the weight
constexpr double kFpfhOne = 1099511627776.0;        // 2^40: the weight's fixed point

// The size of the words.  W <= 2^40 / (2^-20 * n_j) and count <= n_j, so W * count <= 2^60: hi < 2^29, lo < 2^32, and with at most 2^26
// contributing points every sum stays below 2^58.
static_assert(kFpfhMinD2 == 1.0f / 1048576.0f, "the floor of d2 is 2^-20");
static_assert(kFpfhOne * 1048576.0 <= 1152921504606846976.0, "W * count <= 2^60 fits 64 bits");
static_assert(kFpfhMaxPoints <= (1ll << 26), "2^26 terms of hi < 2^29 and of lo < 2^32 stay below 2^58");
static_assert(kFpfhMaxRadius <= kNrmMaxRadius && kFpfhMaxPoints <= kNrmMaxPoints, "the surface is a cloud of the normals");
static_assert(kFpfhDim == 3 * kFpfhBins, "three sub-histograms");

// the edge directions (cos, sin) of -pi + 2 pi k / 11 for k = 1 .. 5; those of k = 6 .. 10 are their mirror images (cos, -sin) of 11 - k
constexpr double kFpfhEdgeC1 = -0.8412535328311811, kFpfhEdgeS1 = -0.5406408174555978;
constexpr double kFpfhEdgeC2 = -0.4154150130018863, kFpfhEdgeS2 = -0.9096319953545184;
constexpr double kFpfhEdgeC3 = 0.14231483827328512, kFpfhEdgeS3 = -0.9898214418809327;
constexpr double kFpfhEdgeC4 = 0.6548607339452851, kFpfhEdgeS4 = -0.7557495743542583;
constexpr double kFpfhEdgeC5 = 0.9594929736144975, kFpfhEdgeS5 = -0.2817325568414295;

// floor((f + 1) * 5.5) clamped to 0 .. 10
LMONO_VM_HD int fpfh_bin(double f)
{
    const double t = (f + 1.0) * 5.5;
    return t >= 10.0 ? 10 : (t >= 1.0 ? (int)t : 0);          // a NaN, which no finite input gives, would land in bin 0
}

// The bin of the direction (x, y): floor(11 (atan2(y, x) + pi) / (2 pi)) clamped to 10, decided by the side of each edge direction e_k the vector
// lies on (e_k x (x, y) = c_k y - s_k x >= 0 iff the angle is at or past edge k, both in the same half plane).  y < 0: angles in (-pi, 0), edges 1 .. 5;
// otherwise angles in [0, pi], bin 5 and edges 6 .. 10.  (0, 0) is bin 5, atan2's 0.  y == -0.0 counts as +0.0.
LMONO_VM_HD int fpfh_angle_bin(double x, double y)
{
    if (x == 0.0 && y == 0.0) return 5;
    if (y < 0.0)
        return (int)(kFpfhEdgeC1 * y - kFpfhEdgeS1 * x >= 0.0) + (int)(kFpfhEdgeC2 * y - kFpfhEdgeS2 * x >= 0.0) + (int)(kFpfhEdgeC3 * y - kFpfhEdgeS3 * x >= 0.0) +
               (int)(kFpfhEdgeC4 * y - kFpfhEdgeS4 * x >= 0.0) + (int)(kFpfhEdgeC5 * y - kFpfhEdgeS5 * x >= 0.0);
    return 5 + (int)(kFpfhEdgeC5 * y + kFpfhEdgeS5 * x >= 0.0) + (int)(kFpfhEdgeC4 * y + kFpfhEdgeS4 * x >= 0.0) + (int)(kFpfhEdgeC3 * y + kFpfhEdgeS3 * x >= 0.0) +
           (int)(kFpfhEdgeC2 * y + kFpfhEdgeS2 * x >= 0.0) + (int)(kFpfhEdgeC1 * y + kFpfhEdgeS1 * x >= 0.0);
}

// The three bins of the pair (i, j), d2 > 0 the caller's test; false: the pair is skipped (|dp x n1| == 0).  b[0]: angle, b[1]: f2, b[2]: f3
LMONO_VM_HD bool fpfh_pair(float pix, float piy, float piz, float nix, float niy, float niz, float pjx, float pjy, float pjz, float njx, float njy, float njz, int b[3])
{
    double d0 = (double)pjx - (double)pix, d1 = (double)pjy - (double)piy, d2 = (double)pjz - (double)piz;
    const double f4 = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double a1 = (((double)nix * d0 + (double)niy * d1) + (double)niz * d2) / f4;
    const double a2 = (((double)njx * d0 + (double)njy * d1) + (double)njz * d2) / f4;
    const bool swap = fabs(a1) < fabs(a2);
    const double n10 = swap ? (double)njx : (double)nix, n11 = swap ? (double)njy : (double)niy, n12 = swap ? (double)njz : (double)niz;
    const double n20 = swap ? (double)nix : (double)njx, n21 = swap ? (double)niy : (double)njy, n22 = swap ? (double)niz : (double)njz;
    if (swap) { d0 = -d0; d1 = -d1; d2 = -d2; }
    const double f3 = swap ? -a2 : a1;
    const double v0 = d1 * n12 - d2 * n11, v1 = d2 * n10 - d0 * n12, v2 = d0 * n11 - d1 * n10;
    const double vn = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    if (vn == 0.0) return false;
    const double u0 = n11 * v2 - n12 * v1, u1 = n12 * v0 - n10 * v2, u2 = n10 * v1 - n11 * v0;
    const double f2 = ((v0 * n20 + v1 * n21) + v2 * n22) / vn;
    const double x = (n10 * n20 + n11 * n21) + n12 * n22, y = ((u0 * n20 + u1 * n21) + u2 * n22) / vn;
    b[0] = fpfh_angle_bin(x, y); b[1] = fpfh_bin(f2); b[2] = fpfh_bin(f3);
    return true;
}

// the integer weight of a surface point at squared distance d2 from the keypoint whose SPFH has nj > 0 pairs
LMONO_VM_HD uint64_t fpfh_weight(float d2, unsigned nj)
{
    const float c = d2 < kFpfhMinD2 ? kFpfhMinD2 : d2;
    return (uint64_t)(kFpfhOne / ((double)c * (double)nj));
}

// what the count `cnt` of one bin adds under the weight W
LMONO_VM_HD void fpfh_add(uint64_t W, unsigned cnt, uint64_t &hi, uint64_t &lo)
{
    const uint64_t P = W * (uint64_t)cnt;
    hi += P >> 32; lo += P & 0xffffffffull;
}

LMONO_VM_HD double fpfh_value(uint64_t hi, uint64_t lo) { return (double)hi * 4294967296.0 + (double)lo; }

// the total of a sub-histogram: its eleven values added in index order
LMONO_VM_HD double fpfh_total(const double *v)
{
    double t = v[0];
    for (int b = 1; b < kFpfhBins; b++) t = t + v[b];
    return t;
}

LMONO_VM_HD float fpfh_scale(double v, double total) { return (float)((v * 100.0) / total); }

// a record with a normal
LMONO_VM_HD bool fpfh_has_normal(float nx) { return nx == nx; }

// The default cell for the radius r at 2 rings: icp_default_cell's rule.  A tuning value: it cannot change a result.
inline float fpfh_default_cell(float radius) { return icp_default_cell(radius); }

// bounds of the parameters (the create function and fpfh_test refuse alike)
LMONO_VM_HD bool fpfh_params_ok(float radius, float cell, int max_rings)
{
    if (!(radius > 0.0f && radius <= kFpfhMaxRadius)) return false;
    if (!(cell > 0.0f) || !(1.0f / cell > 0.0f) || !(1.0f / cell <= 3.0e38f) || max_rings < 1 || max_rings > kSorMaxRings) return false;
    return sor_rho(max_rings, cell) >= radius;
}

} // namespace lmono
