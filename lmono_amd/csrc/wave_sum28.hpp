// Sums over a 64-lane wave of up to 32 doubles per lane at once, host and device (tests/wave_sum28_check.cpp builds this header with
// g++ and runs it over 64 modelled lanes).
//
// wave_sum_d (common.hpp) sums ONE double with a butterfly over the lane pairs of masks 32, 16, 8, 4, 2, 1: six exchanges and six adds,
// and every lane ends with the sum.  k_lm_solve sums 28 doubles (H 21 | g 6 | cost) per sweep and needs each sum in one lane only, so 28
// butterflies exchange and add six times what is used.  wave_sum28_scatter is the reduce-scatter over the same pairs in the same order:
// at mask 32 a lane keeps 16 of its 32 slots and hands the partner the other 16, at masks 16, 8, 4, 2 it keeps 8, 4, 2, 1, and at mask 1
// both lanes of a pair add the one slot left: 16 + 8 + 4 + 2 + 1 + 1 = 32 exchanges and adds instead of 28 x 6 = 168.
//
// The bytes.  At every stage the value a lane keeps for a slot is its own partial plus the partner's partial of the same slot -- the two
// operands the butterfly adds in that lane at that stage -- so by induction over the stages, and because IEEE addition commutes, every
// kept double equals the butterfly's bit for bit (two NaNs of different payloads aside: which payload survives depends on operand order).
//
// Where a sum ends up: a lane with bit `mask` clear keeps the lower half of its slots, so the slot's index is the lane's bits 5..1:
// lanes 2 i and 2 i + 1 both end with slot i, in v[0].
//
// Every slot index below is a compile-time constant (the loops unroll, the stages are template arguments): a lane-dependent index would
// put the array in scratch or LDS.
//
// The lanes are a policy L over the value type T (double on the device, 64 doubles side by side in the host model):
//   L::pick<kMask>(a, b)   a in lanes whose bit kMask is clear, b in the others
//   L::xchg<kMask>(a)      the partner's a (partner = lane ^ kMask)
//   L::swap<kMask>(a, b)   lanes with the bit clear: b <- partner's a;  lanes with the bit set: a <- partner's b   (v_permlane32_swap /
//                          v_permlane16_swap: one instruction per dword moves both directions and needs no select)
#pragma once

#if defined(__HIPCC__)
#define LMONO_WS28_HD __host__ __device__ __forceinline__
#else
#define LMONO_WS28_HD inline
#endif

namespace lmono {

// one stage by swap: afterwards v[j], j < kHalf, holds own + partner's partial of the slot this lane keeps
template <int kMask, int kHalf, class L, class T>
LMONO_WS28_HD void ws28_stage_swap(const L &lanes, T *v)
{
#pragma unroll
    for (int j = 0; j < kHalf; j++) {
        lanes.template swap<kMask>(v[j], v[j + kHalf]);
        v[j] = v[j] + v[j + kHalf];
    }
}

// one stage by select and exchange
template <int kMask, int kHalf, class L, class T>
LMONO_WS28_HD void ws28_stage_xchg(const L &lanes, T *v)
{
#pragma unroll
    for (int j = 0; j < kHalf; j++) {
        const T keep = lanes.template pick<kMask>(v[j], v[j + kHalf]);
        const T send = lanes.template pick<kMask>(v[j + kHalf], v[j]);
        v[j] = keep + lanes.template xchg<kMask>(send);
    }
}

// v[0 .. 31]: this lane's partials of slots 0 .. 31 (unused slots: any finite value, 0).  Afterwards v[0] of lanes 2 i and 2 i + 1 is the
// wave's sum of slot i, added in wave_sum_d's order; v[1 ..] are scratch.
template <class L, class T>
LMONO_WS28_HD void wave_sum28_scatter(const L &lanes, T *v)
{
    ws28_stage_swap<32, 16>(lanes, v);
    ws28_stage_swap<16, 8>(lanes, v);
    ws28_stage_xchg<8, 4>(lanes, v);
    ws28_stage_xchg<4, 2>(lanes, v);
    ws28_stage_xchg<2, 1>(lanes, v);
    v[0] = v[0] + lanes.template xchg<1>(v[0]);
}

#if defined(__HIPCC__)
// The lanes of a gfx950 wave.  Masks 32 and 16: v_permlane32_swap / v_permlane16_swap (VALU, both directions in one instruction).
// Masks 8, 2, 1: DPP row_ror:8 and quad_perm (VALU moves).  Mask 4 has no DPP pattern: ds_swizzle (the LDS crossbar, but no address
// register and no LDS memory).  All lanes of the wave must be active.
struct Ws28Wave {
    int lane;
    template <int kMask> __device__ __forceinline__ double pick(double a, double b) const { return (lane & kMask) ? b : a; }
    template <int kMask> __device__ __forceinline__ static unsigned int xchg32(unsigned int u)
    {
        static_assert(kMask == 8 || kMask == 4 || kMask == 2 || kMask == 1, "the masks the scatter exchanges by moves");
        if (kMask == 8) return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)u, 0x128, 0xf, 0xf, false);      // row_ror:8
        if (kMask == 4) return (unsigned int)__builtin_amdgcn_ds_swizzle((int)u, 0x101f);                           // and 0x1f, or 0, xor 4
        if (kMask == 2) return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)u, 0x4e, 0xf, 0xf, false);       // quad_perm:[2,3,0,1]
        return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)u, 0xb1, 0xf, 0xf, false);                       // quad_perm:[1,0,3,2]
    }
    template <int kMask> __device__ __forceinline__ double xchg(double a) const
    {
        const unsigned long long u = (unsigned long long)__double_as_longlong(a);
        const unsigned int lo = xchg32<kMask>((unsigned int)u), hi = xchg32<kMask>((unsigned int)(u >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    template <int kMask> __device__ __forceinline__ void swap(double &a, double &b) const
    {
        static_assert(kMask == 32 || kMask == 16, "the masks that have a swap instruction");
        const unsigned long long ua = (unsigned long long)__double_as_longlong(a), ub = (unsigned long long)__double_as_longlong(b);
        unsigned int alo = (unsigned int)ua, ahi = (unsigned int)(ua >> 32), blo = (unsigned int)ub, bhi = (unsigned int)(ub >> 32);
        if (kMask == 32) {
            const auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
            const auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
            alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
        } else {
            const auto l = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
            const auto h = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
            alo = l[0]; blo = l[1]; ahi = h[0]; bhi = h[1];
        }
        a = __longlong_as_double((long long)(((unsigned long long)ahi << 32) | alo));
        b = __longlong_as_double((long long)(((unsigned long long)bhi << 32) | blo));
    }
};
#endif

}  // namespace lmono

#undef LMONO_WS28_HD
