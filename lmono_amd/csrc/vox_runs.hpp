// Run lengths of k_voxel's segments, host and device (tests/vox_runs_check.cpp builds this header with g++).
//
// k_voxel keeps "point i continues the run of point i - 1" as a bitmap, one 64-bit word per 64 ring points.  The run that
// starts at point i0 (a segment head, its own bit is 0) covers i0 and every following point whose bit is set, so its length
// is 1 + the number of consecutive ones from bit i0 + 1 on.  vox_run_length reads that from a 64-bit window of two
// neighbouring words and a count of trailing ones; a run that fills the whole window moves the window on by 64 bits.
//
// Contract of the bitmap: every run ends in a 0 bit inside the bitmap's words, and two zero words follow the last word
// that can hold a point (the window of the last points, and the step past a full window, read them).
#pragma once

#if defined(__HIPCC__)
#define LMONO_VOX_HD __host__ __device__ __forceinline__
#else
#define LMONO_VOX_HD inline
#endif

// consecutive one bits of w from bit 0 upwards (0..64)
LMONO_VOX_HD int vox_trailing_ones(unsigned long long w)
{
    const unsigned long long z = ~w;
    return z ? __builtin_ctzll(z) : 64;
}

// bits p .. p + 63 of the bitmap as one word (bit k of the result = bit p + k of the bitmap)
LMONO_VOX_HD unsigned long long vox_window(const unsigned long long *bits, int p)
{
    const int w = p >> 6, sh = p & 63;
    const unsigned long long a = bits[w], b = bits[w + 1];
    return sh ? (a >> sh) | (b << (64 - sh)) : a;
}

// length of the run whose head is point i0
LMONO_VOX_HD int vox_run_length(const unsigned long long *contw, int i0)
{
    int p = i0 + 1;
    int n = vox_trailing_ones(vox_window(contw, p));
    int rl = 1 + n;
    while (n == 64) {            // the run passes the window: 64 points further on
        p += 64;
        n = vox_trailing_ones(vox_window(contw, p));
        rl += n;
    }
    return rl;
}
