// Trigger clustering of the search pipeline on the device.
//
// Reference: MLGWSC-1/inference.py:140-166 (`get_clusters`) fed by :484-487 (`evaluate_slices` keeps the windows whose
// score exceeds `trigger_threshold`, one `.item()` per window): time-ordered triggers closer than `cluster_threshold`
// seconds to their predecessor join its cluster; a cluster is reported as the time and value of its FIRST maximum.
// Here the per-window scores never leave the GPU before they are clustered: one wave walks the score array 64 windows at a
// time, the trigger mask of a step is a ballot, and the (rare) set bits are folded into a wave-uniform running cluster --
// a sequential algorithm whose state is four scalars, so one wave is the natural shape; n / 64 steps of a few
// instructions (120 000 windows: about 2 000 steps).  Times are the reference's float64 stamps, compared in float64.
#include "cluster_wave.h"

namespace gww {
namespace {

// the wave loop itself: cluster_wave.h (shared with the time slides, timeslide.hip)
__global__ __launch_bounds__(64) void k_cluster_triggers(const double* __restrict__ times, const float* __restrict__ scores,
                                                         long n, float trigger_threshold, double cluster_threshold,
                                                         double* __restrict__ out_t, float* __restrict__ out_v,
                                                         int* __restrict__ out_count, int max_clusters) {
  cluster_wave(times, scores, n, trigger_threshold, cluster_threshold, out_t, out_v, out_count, max_clusters);
}

}  // namespace
}  // namespace gww

using namespace gww;

extern "C" int gww_cluster_triggers_f64(const double* times, const float* scores, long n, float trigger_threshold,
                                        double cluster_threshold, double* out_times, float* out_vals, int* out_count,
                                        int max_clusters, void* stream) {
  GWW_REQUIRE(out_count && (n == 0 || (times && scores)) && (max_clusters == 0 || (out_times && out_vals)),
              "gww_cluster_triggers_f64: NULL argument");
  GWW_REQUIRE(n >= 0 && max_clusters >= 0, "gww_cluster_triggers_f64: negative size");
  hipLaunchKernelGGL(k_cluster_triggers, dim3(1), dim3(64), 0, (hipStream_t)stream, times, scores, n, trigger_threshold,
                     cluster_threshold, out_times, out_vals, out_count, max_clusters);
  GWW_LAUNCH_CHECK();
  return GWW_OK;
}
