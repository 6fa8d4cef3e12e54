// k_wf_merge: makes the late rounds' thinned-out tasks of a wavefront batch dense before k_wf_tail takes them over (DESIGN.md 4.1,
// "the merged tail"; scheduled by launch_wavefront in hrt_hip.hip).  A unit of its own: the resource report of hrt_hip.hip's kernels is
// pinned kernel by kernel (tests/test_*_resources.py), this kernel's by tests/test_merge_resources.py.
//
// Large batches have more tasks than k_wf_tail keeps waves resident (the headline frame: 16 000 on 4096), so a tail wave would
// run ~4 tasks one after the other, each a chain of ~30 rounds x (one ray's traversal + a partly filled shade chunk).  This
// kernel makes them dense first: every K neighbouring tasks become ONE task of K x T positions, so that there are no more
// tasks than tail waves and a wave's per-round chain is shared by K times as many rays.  It runs between round R's last
// k_wf_ext and round R's shading: the traversal records E0..E3, qn and rn are consumed by then, only the state of parity
// R & 1 is live (S0..S3, the traversal's hit already in S2), and k_wf_tail entered with qn = rn = 0 shades round R first.
// One wave per merged task m: the live[t] records of the old tasks t = mK, mK + 1, ... move, in that order, from [t T, ...)
// to [m K T + (the live records of the tasks before t), ...), IN PLACE and 64 positions per step.  Why that is safe:
//   * the destination never lies above the source: the j tasks before task mK + j hold at most j T records;
//   * the 64 loads of a step are one instruction per array, and the stores depend on them: all are read before any is written;
//   * a step's stores end at destination + 64 <= source + 64 = the first position the next step reads: nothing unread is hit;
//   * a wave only touches the segment [m K T, (m + 1) K T) of its own merged task;
//   * while every earlier task is full, destination == source and there is nothing to move.
// Paths are addressed by the slot they carry in S2.w (RNG context, rad[slot], the sample-ordered reduce): where a record lies
// shows nowhere in the film.  The merged counts go to a SECOND set of per-task arrays -- in place, wave 1 would overwrite
// live[1] while wave 0 still reads it -- which the host hands to k_wf_tail as its live / qn / rn.
// No LDS, no communication between waves, no loop that waits for another wave.
#include <hip/hip_runtime.h>

namespace {
// a per-task count: the same in every lane, but loaded through a vector load -- tell the compiler (loop bounds in SGPRs)
__device__ inline unsigned uniform(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }

__global__ __launch_bounds__(256) void k_wf_merge(float4* s0, float4* s1, float4* s2, float* s3, const unsigned* __restrict__ live, unsigned T, unsigned n_tasks,
                                                  unsigned K, unsigned n_merged, unsigned* __restrict__ live_m, unsigned* __restrict__ qn_m, unsigned* __restrict__ rn_m) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned m = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (m >= n_merged) return;
    const unsigned first = m * K, last = first + K < n_tasks ? first + K : n_tasks;
    const unsigned base = first * T;
    unsigned total = 0;
    for (unsigned t = first; t < last; ++t) {
        const unsigned n = uniform(live[t]);
        const unsigned src = t * T, dst = base + total;
        if (dst != src) {
            for (unsigned j0 = 0; j0 < n; j0 += 64) {
                const bool mine = j0 + lane < n;
                float4 a = make_float4(0, 0, 0, 0), b = a, c = a;
                float az = 0.0f;
                if (mine) { a = s0[src + j0 + lane]; b = s1[src + j0 + lane]; c = s2[src + j0 + lane]; az = s3[src + j0 + lane]; }
                if (mine) { s0[dst + j0 + lane] = a; s1[dst + j0 + lane] = b; s2[dst + j0 + lane] = c; s3[dst + j0 + lane] = az; }
            }
        }
        total += n;
    }
    if (lane == 0) { live_m[m] = total; qn_m[m] = 0; rn_m[m] = 0; }
}
}  // namespace

// The state arrays of one parity (WfBuf::S0..S3[par]) and the batch's task counts; K tasks become one, n_merged = ceil(n_tasks / K).
extern "C" __attribute__((visibility("hidden"))) void hrt_wf_merge_launch(float4* s0, float4* s1, float4* s2, float* s3, const unsigned* live, unsigned T,
                                                                          unsigned n_tasks, unsigned K, unsigned* live_m, unsigned* qn_m, unsigned* rn_m,
                                                                          hipStream_t stream) {
    const unsigned n_merged = (n_tasks + K - 1) / K;
    hipLaunchKernelGGL(k_wf_merge, dim3((n_merged + 3) / 4), dim3(256), 0, stream, s0, s1, s2, s3, live, T, n_tasks, K, n_merged, live_m, qn_m, rn_m);
}
