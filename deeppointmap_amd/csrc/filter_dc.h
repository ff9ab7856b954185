// What dpm_outlier_filter_dc / dpm_lowpass_filter_dc (knn.hip, where the grid build and the neighbour search live) need
// from preprocess.hip, where the similarity and the statistical cut live: the device-count launches of those two kernels.
// Library-internal: not part of the C ABI.
#pragma once
#include "dpm_common.h"

constexpr int DPM_FILTER_FLUX_MAX = 8;  // the descending list lowpass_sim_kernel keeps in registers

namespace dpm_detail {
// sim[i] for i < count[0] (clamped to [0, cap]); nothing when that is <= K
__attribute__((visibility("hidden"))) void launch_lowpass_sim_dc(const float *normals, const int32_t *idx, const int32_t *count,
                                                                 int cap, int K, int flux, float *sim, hipStream_t st);
// the cut over stat[0 .. count[0]) and the stable compaction; a frame of at most kmin points passes through
__attribute__((visibility("hidden"))) void launch_stat_filter_dc(const float *stat, const int32_t *count, int cap, int kmin,
                                                                 float k_std, int mode, float ratio, const float *xyz_in,
                                                                 const int32_t *idx_in, float *xyz_out, int32_t *idx_out,
                                                                 int32_t *count_out, hipStream_t st);
}  // namespace dpm_detail
