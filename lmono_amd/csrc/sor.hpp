// sor.hpp -- the arithmetic of the statistical outlier removal in front of the voxel map: validity, distance, score,
// statistics, threshold and keep test.  One text for the kernels (sor.hip) and for a CPU program (host/sor_test.cpp); every float
// operation is a single IEEE operation (build with -ffp-contract=off).  The stage is the pcl::StatisticalOutlierRemoval<pcl::PointXYZRGB>
// (setMeanK(100), setStddevMulThresh(1.0)) that MapBuilder::processMapping carries commented out (Map_Builder.cc:24-29).  Its definition
// here is this project's own and differs from PCL's in three ways: a point with fewer than k neighbours within rho = (R - 0.25) h is an
// outlier by definition (PCL looks as far as it must), the sum of the k distances is a 2^-16 m fixed-point integer (so the statistics are
// exact integers and any reduction order gives the same words), and the result is a pure function of the SET of input points.
//
// Why the grid cannot change the result.  The grid (cells of side h keyed by vm_key, rings of Chebyshev cell distance) is only how the
// neighbours are found.  A search that has looked at all cells within ring r >= 1 of the query's cell may stop as soon as it holds k values
// with d2 <= sor_rho2(r, h) = (((float)r - 0.25f) * h)^2: a point in an unvisited cell differs from the query by more than r in the COMPUTED
// t = x * inv of some axis (their floors differ by more than r).  t carries at most 2^-24 * 2^20 = 2^-4 of rounding per point, so the real
// separation on that axis exceeds (r - 0.125) h, which is more than 0.7 % above (r - 0.25) h for every r <= 64 -- far above the float32
// roundings of d2 (a few 2^-24 relative).  So every point outside the visited cube has d2 > sor_rho2(r, h), and the k smallest values
// are all inside.  At r = R the same argument shows that { j : d2 <= rho2 } is complete.
#pragma once
#include "voxel_map.hpp"

namespace lmono {

constexpr int kSorMaxK = 128, kSorMaxRings = 64;
constexpr float kSorMaxRho = 256.0f;
constexpr uint32_t kSorNoScore = 0xffffffffu;       // v of a rejected or isolated point

// (((float)r - 0.25f) * h)^2: the stopping bound of ring r, and rho2 at r = max_rings
LMONO_VM_HD float sor_rho(int r, float h) { return ((float)r - 0.25f) * h; }
LMONO_VM_HD float sor_rho2(int r, float h) { const float rho = sor_rho(r, h); return rho * rho; }

// valid iff the voxel map's cell function accepts the point at inv = 1.0f / h; c[3] is its cell
LMONO_VM_HD bool sor_cell(float x, float y, float z, float inv, uint64_t &key, int c[3])
{
    int q;
    if (!vm_axis(x, inv, c[0], q) || !vm_axis(y, inv, c[1], q) || !vm_axis(z, inv, c[2], q)) return false;
    key = vm_key(c[0], c[1], c[2]);
    return true;
}

LMONO_VM_HD float sor_d2(float xi, float yi, float zi, float xj, float yj, float zj)
{
    const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return (dx * dx + dy * dy) + dz * dz;
}

// one distance in units of 2^-32 m: correctly rounded float32 root, exact product in fp64, truncated
LMONO_VM_HD uint64_t sor_u(float d2) { return (uint64_t)((double)sqrtf(d2) * 4294967296.0); }

// the score of a point from the exact sum S of its k values u: the sum of the k distances in units of 2^-16 m (< 2^31)
LMONO_VM_HD uint32_t sor_v(uint64_t S) { return (uint32_t)(S >> 16); }

// what one scored point adds to the statistics A, Bhi, Blo
LMONO_VM_HD void sor_terms(uint32_t v, uint64_t &a, uint64_t &bhi, uint64_t &blo)
{
    const uint64_t vv = (uint64_t)v * (uint64_t)v;
    a = v; bhi = vv >> 32; blo = vv & 0xffffffffull;
}

// mean, sqrt(var) and the threshold in v units from the four exact words; M = 0 gives zeros (nothing is scored, nothing kept)
LMONO_VM_HD double sor_threshold(uint64_t M, uint64_t A, uint64_t Bhi, uint64_t Blo, double mul, double &mean, double &sd)
{
    mean = 0.0; sd = 0.0;
    if (M == 0) return 0.0;
    mean = (double)A / (double)M;
    double var = 0.0;
    if (M > 1) {
        const double e2 = ((double)Bhi * 4294967296.0 + (double)Blo) / (double)M;
        const double mm = mean * mean;
        var = (e2 - mm) * ((double)M / (double)(M - 1));
        if (!(var > 0.0)) var = 0.0;
    }
    sd = sqrt(var);
    const double t = mul * sd;
    return mean + t;
}

LMONO_VM_HD bool sor_keep(uint32_t v, double thr) { return v != kSorNoScore && (double)v <= thr; }

} // namespace lmono
