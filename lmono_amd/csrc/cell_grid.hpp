// cell_grid.hpp -- the origin and span rules of a cell grid with an origin (cell_grid.hip): the ICP's target and the cloud of the surface
// normals.  One text for the grid's kernels and for the CPU programs (host/icp_test.cpp, host/normals_test.cpp).  A point is valid iff sor_cell
// accepts it; the origin o[a] = (min_a + max_a) * 0.5f over the valid points, min and max in the order of icp_ord; a valid point with some
// |p_a - o_a| >= kIcpSpan is out of span.
#pragma once
#include "sor.hpp"

namespace lmono {

constexpr float kIcpSpan = 2048.0f;             // |w_a|, |u_a| stay below it: 2^-16 m fixed point in 28 bits

// the order of min / max for the origin: float order with -0 below +0, as unsigned integers
LMONO_VM_HD uint32_t icp_ord(float x)
{
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LMONO_VM_HD float icp_unord(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    __builtin_memcpy(&x, &b, 4);
    return x;
}
LMONO_VM_HD float icp_origin(float mn, float mx) { return (mn + mx) * 0.5f; }

// centred coordinate in range: finite and |c| < 2048
LMONO_VM_HD bool icp_in_span(float c) { return c > -kIcpSpan && c < kIcpSpan; }

} // namespace lmono
