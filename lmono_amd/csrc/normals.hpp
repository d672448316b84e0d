// normals.hpp -- the arithmetic of the surface normals and curvature of a cloud: the pcl::NormalEstimation with
// setRadiusSearch(0.05) that opens MapBuilder::alignmentToMap, the coarse map-to-map alignment the reference carries commented out
// (mono_lidar_mapping/src/map_builder/Map_Builder.cc:110-210), and that every later stage of that function consumes.  One text for the kernels
// (normals.hip), for a CPU program (host/normals_test.cpp) and for the host side of the C ABI; every float operation is a single IEEE operation
// (build with -ffp-contract=off).  The definition is this project's own: a point's record is a pure function of the SET of input points and of
// the point itself.  Parity with PCL is unpinned.
//
// Valid points, origin, span: the rules of a grid with an origin (cell_grid.hpp), as the ICP's target.  A point is valid iff sor_cell accepts it at inv = 1.0f / h; the origin
// o[a] = (min_a + max_a) * 0.5f over the valid points in the order of icp_ord; w = p - o; a valid point with some |w_a| >= 2048 is out of span.
// An invalid or out-of-span point is rejected: counted, never a neighbour, and its record is four NaNs (kNrmNaN) with count 0.  iw_a = nrm_fix(w_a).
// Neighbourhood of i: every non-rejected j, i itself and every duplicate included, with sor_d2(p_i, p_j) <= r * r in float32; N of them.
// Sums about the query point, d = iw_j - iw_i: N, S[a] = sum d_a, SS[ab] = sum d_a d_b for a <= b (NrmSums).  All exact integers, so no
// order of the neighbours, of the cells or of a reduction can change a word.
// Solve (nrm_solve), when N >= min_neighbours: C_ab = (double)SS_ab - ((double)S_a * (double)S_b) / (double)N (the scatter matrix, not divided
// by N); rej_jacobi<3>, kNrmSweeps sweeps; b = rej_smallest<3> (a tie goes to the lowest index); v = column b of V over its norm;
// curvature = lambda / tr with lambda = C_bb > 0 ? C_bb : 0 and tr = (C_00 + C_11) + C_22 after the sweeps, 0 when tr is not positive.  A
// neighbourhood of duplicates alone has C = 0: V = I, b = 0, the normal (1, 0, 0), curvature 0.
// Orientation: with a viewpoint vp, dot = ((vp_x - p_x) v0 + (vp_y - p_y) v1) + (vp_z - p_z) v2 in fp64, and v is negated iff dot < 0.  Without
// a viewpoint, or when dot == 0, the sign is canonical: the component of largest magnitude (the lowest index among equals) is made positive.
// Then 0.0 is added to each component, so that no -0.0 reaches the output.  The record is the (float) of each fp64 value.
// With N < min_neighbours the record is four NaNs and the count is N.
//
// Why the grid cannot change the result: the argument at the head of sor.hpp.  The grid (cells of side h keyed by vm_key) is only how the
// neighbours are found.  A point in a cell outside ring R of the query's cell differs from the query by more than R in the computed t = x * inv of
// some axis; t carries at most 2^-4 of rounding per point, so the real separation on that axis exceeds (R - 0.125) h, more than 0.7 % above
// sor_rho(R, h) = (R - 0.25) h -- far above the float32 roundings of d2.  So every point outside the cube has d2 > sor_rho2(R, h), and with
// sor_rho(R, h) >= r (float32 rounding is monotone: sor_rho2 >= r * r) the set { j : d2 <= r * r } lies inside the cube whole.
#pragma once
#include "cell_grid.hpp"
#include "icp.hpp"

namespace lmono {

constexpr int kNrmSweeps = 8;                       // cyclic Jacobi sweeps of the 3 x 3 problem (the off-diagonal is exactly 0 on the planes of tests/test_normals_ref_cpu.py)
constexpr float kNrmMaxRadius = 4.0f;
constexpr long long kNrmMaxPoints = 1ll << 26;
constexpr int kNrmWords = 10;                       // of NrmSums
constexpr uint32_t kNrmNaN = 0x7fc00000u;           // every float of a record without a normal

// The size of the words.  A neighbour has d2 <= r * r <= 16 in float32, so the real |x_j - x_i| < 4 + 2^-19 (the roundings of dx, of the squares
// and of the sums are a few 2^-24 relative).  w = p - o is rounded to float32 below 2048: at most 2^-14 m per point.  So 65536 |w_j - w_i| <
// 2^18 + 16, and the two truncations of nrm_fix add less than 1 each: |d_a| < kNrmMaxD.  A product stays below 2^37, and with N <= 2^26 every
// word below 2^63.
constexpr long long kNrmMaxD = (1ll << 18) + 32;
static_assert(kNrmMaxRadius * 65536.0f + 32.0f <= (float)kNrmMaxD, "kNrmMaxD covers the radius");
static_assert(kNrmMaxD * kNrmMaxD < (1ll << 37), "a product d_a d_b stays below 2^37");
static_assert(kNrmMaxPoints <= (1ll << (63 - 37)), "N products stay below 2^63");
static_assert(kNrmMaxRadius <= kIcpMaxCorr, "the grid of the ICP's target serves the radius");

struct NrmSums { long long N, S[3], SS[6]; };      // SS: xx, xy, xz, yy, yz, zz
static_assert(sizeof(NrmSums) == 8 * kNrmWords, "NrmSums layout");

struct NrmRecord { float nx, ny, nz, curvature; };
static_assert(sizeof(NrmRecord) == 16, "NrmRecord layout");

// icp_fix of an in-span coordinate: |c * 65536| < 2^27, so the value fits 32 bits
LMONO_VM_HD int nrm_fix(float c) { return (int)((double)c * 65536.0); }

// what the neighbour with centred fixed-point coordinates jw adds to the sums of the query point iw
LMONO_VM_HD void nrm_add(const int iw[3], const int jw[3], NrmSums &s)
{
    const int dx = jw[0] - iw[0], dy = jw[1] - iw[1], dz = jw[2] - iw[2];
    s.N += 1;
    s.S[0] += dx; s.S[1] += dy; s.S[2] += dz;
    s.SS[0] += (long long)dx * dx; s.SS[1] += (long long)dx * dy; s.SS[2] += (long long)dx * dz;
    s.SS[3] += (long long)dy * dy; s.SS[4] += (long long)dy * dz; s.SS[5] += (long long)dz * dz;
}

// the record of the point p from its finished sums (N >= min_neighbours is the caller's test); vp: the viewpoint or nullptr;
// swept (optional, [9]): the scatter matrix as the sweeps leave it, for the check that they diagonalise it
LMONO_VM_HD NrmRecord nrm_solve(const NrmSums &s, float px, float py, float pz, const float *vp, double *swept = nullptr)
{
    const double n = (double)s.N;
    const double S0 = (double)s.S[0], S1 = (double)s.S[1], S2 = (double)s.S[2];
    double C[9], V[9];
    C[0] = (double)s.SS[0] - (S0 * S0) / n; C[1] = (double)s.SS[1] - (S0 * S1) / n; C[2] = (double)s.SS[2] - (S0 * S2) / n;
    C[4] = (double)s.SS[3] - (S1 * S1) / n; C[5] = (double)s.SS[4] - (S1 * S2) / n; C[8] = (double)s.SS[5] - (S2 * S2) / n;
    C[3] = C[1]; C[6] = C[2]; C[7] = C[5];
    rej_jacobi<3>(C, V, kNrmSweeps);
    if (swept) for (int e = 0; e < 9; e++) swept[e] = C[e];
    const int b = rej_smallest<3>(C);
    // column b and C_bb by selects, not by an index: a private array indexed by a variable leaves the registers
    double v0 = b == 0 ? V[0] : (b == 1 ? V[1] : V[2]), v1 = b == 0 ? V[3] : (b == 1 ? V[4] : V[5]), v2 = b == 0 ? V[6] : (b == 1 ? V[7] : V[8]);
    const double nrm = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    v0 = v0 / nrm; v1 = v1 / nrm; v2 = v2 / nrm;
    const double cbb = b == 0 ? C[0] : (b == 1 ? C[4] : C[8]), lambda = cbb > 0.0 ? cbb : 0.0, tr = (C[0] + C[4]) + C[8];
    const double curv = tr > 0.0 ? lambda / tr : 0.0;
    double dot = 0.0;
    if (vp) dot = (((double)vp[0] - (double)px) * v0 + ((double)vp[1] - (double)py) * v1) + ((double)vp[2] - (double)pz) * v2;
    bool flip = dot < 0.0;
    if (dot == 0.0) {
        const double a0 = fabs(v0), a1 = fabs(v1), a2 = fabs(v2);
        double big = v0, ab = a0;
        if (a1 > ab) { big = v1; ab = a1; }
        if (a2 > ab) { big = v2; ab = a2; }
        flip = big < 0.0;
    }
    if (flip) { v0 = -v0; v1 = -v1; v2 = -v2; }
    NrmRecord r;
    r.nx = (float)(v0 + 0.0); r.ny = (float)(v1 + 0.0); r.nz = (float)(v2 + 0.0); r.curvature = (float)curv;
    return r;
}

LMONO_VM_HD NrmRecord nrm_no_normal()
{
    float q;
    const uint32_t b = kNrmNaN;
    __builtin_memcpy(&q, &b, 4);
    NrmRecord r;
    r.nx = q; r.ny = q; r.nz = q; r.curvature = q;
    return r;
}

// The default cell for the radius r at 2 rings: icp_default_cell's rule (the smallest float32 h >= r / 1.75f with sor_rho(2, h) >= r).  A tuning
// value: it cannot change a result.
inline float nrm_default_cell(float radius) { return icp_default_cell(radius); }

// bounds of the parameters (the create function and normals_test refuse alike)
LMONO_VM_HD bool nrm_params_ok(float radius, int min_neighbours, float cell, int max_rings)
{
    if (!(radius > 0.0f && radius <= kNrmMaxRadius) || min_neighbours < 3) return false;
    if (!(cell > 0.0f) || !(1.0f / cell > 0.0f) || !(1.0f / cell <= 3.0e38f) || max_rings < 1 || max_rings > kSorMaxRings) return false;
    return sor_rho(max_rings, cell) >= radius;
}

} // namespace lmono
