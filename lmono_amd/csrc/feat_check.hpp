// feat_check.hpp -- host-side structural validation of the per-track descriptors (lmono_triangulate, lmono_outlier_scores, lmono_shift_depth_batch).
// Plain C++, no HIP: feat_abi.hip runs it before any upload or launch, and oracle/cpu_shim.cpp (the CPU twin of these entry points) includes this very
// file, so the two refuse the same calls with the same words.  The conditions are the ones stated beside the declarations in include/lmono_hip.h.
#pragma once

namespace lmono {

constexpr int kFeatFrames = 11;      // frames of a window: Rs [11][9], Ps [11][3]

// nullptr: well-formed; otherwise what is wrong (a string literal).  Pointers are the caller's to check.
static inline const char *feat_check_tracks(int n_windows, const int *feat_off, const int *start_frame, const int *obs_off, int track_cnt)
{
    if (track_cnt < 1) return "track_cnt must be >= 1";
    if (feat_off[0] != 0) return "feat_off[0] must be 0";
    for (int w = 0; w < n_windows; w++) if (feat_off[w + 1] < feat_off[w]) return "feat_off must ascend";
    const int F = feat_off[n_windows];
    if (F > 0 && obs_off[0] < 0) return "obs_off must not be negative";
    for (int f = 0; f < F; f++) {
        const int nobs = obs_off[f + 1] - obs_off[f];
        if (nobs < 0) return "obs_off must ascend";
        if (start_frame[f] < 0) return "start_frame must not be negative";
        if (nobs > 0 && start_frame[f] > kFeatFrames - nobs) return "a track's observations must end within the window's 11 frames (start_frame + nobs <= 11)";
    }
    return nullptr;
}

static inline const char *feat_check_refine(int window_size, int refine_max_iter, int iter_cap)
{
    if (window_size < 0 || window_size > kFeatFrames - 1) return "window_size must be 0..10";
    if (refine_max_iter > iter_cap) return "refine_max_iter is above LMONO_FEAT_MAX_REFINE_ITER";
    return nullptr;
}

static inline const char *feat_check_offsets(int n_windows, const int *off)
{
    if (off[0] != 0) return "track offsets must start at 0";
    for (int w = 0; w < n_windows; w++) if (off[w + 1] < off[w]) return "track offsets must ascend";
    return nullptr;
}

} // namespace lmono
