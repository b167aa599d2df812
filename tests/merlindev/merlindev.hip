// merlindev.hip -- TEST-ONLY device build of the transcript layer (merlin.cuh, unchanged) behind the script interpreter of
// transcript_script.cuh: one script per launch, uniform over it, and one case (one message area) per lane.  Built by the Makefile next
// to it (run by build()) with the product's compiler flags into tests/merlindev/libmerlindev.so; the product never loads it.
//
// The STROBE state lives where the product keeps it: a word-interleaved LDS column per lane, behind
//   policy 0: LdsState of device_io.cuh itself (stride NT, the column of k_hash and of the prover kernels);
//   policy 1: a policy of stride 64, the stride of k_ballot_small's state (latency_kernels.cuh: SM_LANES).  That header cannot be included without
//             the whole engine (kernels.cuh, host_plan.hpp), so the policy is restated here.
// A script needs two transcripts (export -> import, clone), so a block runs half as many lanes as its stride and gives each lane two
// columns of the one [50][stride] array.
#include <hip/hip_runtime.h>
#include "../../elastic_elgamal_amd/csrc/device_io.cuh"
#include "transcript_script.cuh"

using namespace eg;

constexpr int MD_SM_LANES = 64;            // = SM_LANES of latency_kernels.cuh (tests/test_gpu_transcript_positions.py compares)
struct Lds64State {
  u32* base;
  __device__ __forceinline__ u32 rd(int i) const { return base[i * MD_SM_LANES]; }
  __device__ __forceinline__ void wr(int i, u32 v) { base[i * MD_SM_LANES] = v; }
};

template <class S, int STRIDE>
__global__ void __launch_bounds__(STRIDE / 2) k_script(const u32* __restrict__ blob, int n, const u32* __restrict__ msgs, u32 msg_words,
                                                        u32* __restrict__ out, u32 out_words) {
  __shared__ u32 lds[50 * STRIDE];
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  Transcript<S> a, b;
  a.st.base = lds + threadIdx.x;
  b.st.base = lds + STRIDE / 2 + threadIdx.x;
  ts_run(a, b, blob, msgs + (size_t)msg_words * i, out + (size_t)out_words * i);
}

// Runs n cases of one script.  Returns 0 or the first failing HIP status (hipErrorInvalidValue for a script that does not fit its
// buffers: nothing is launched then); *step says which call it came from (1 malloc, 2 copy in, 3 memset, 4 launch, 5 synchronise,
// 6 copy out, 7 free).
extern "C" int md_run_script(int policy, const uint32_t* blob, size_t blob_bytes, int n, const uint32_t* msgs, size_t msg_bytes,
                             uint32_t* out, size_t out_words, int* step) {
  *step = 0;
  const long need = ts_out_words(blob, blob_bytes, msg_bytes);
  if (policy < 0 || policy > 1 || n <= 0 || n > (1 << 20) || !msgs || !out || need <= 0 || (size_t)need != out_words)
    return (int)hipErrorInvalidValue;
  const size_t in_bytes = msg_bytes * (size_t)n, out_bytes = sizeof(u32) * out_words * (size_t)n;
  u32 *d_blob = nullptr, *d_in = nullptr, *d_out = nullptr;
  hipError_t e;
  *step = 1;
  if ((e = hipMalloc(&d_blob, blob_bytes)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d_in, in_bytes)) != hipSuccess) { (void)hipFree(d_blob); return (int)e; }
  if ((e = hipMalloc(&d_out, out_bytes)) != hipSuccess) { (void)hipFree(d_blob); (void)hipFree(d_in); return (int)e; }
  do {
    *step = 2;
    if ((e = hipMemcpy(d_blob, blob, blob_bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    if ((e = hipMemcpy(d_in, msgs, in_bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    *step = 3;
    if ((e = hipMemset(d_out, 0, out_bytes)) != hipSuccess) break;
    *step = 4;
    const int block = (policy == 0 ? NT : MD_SM_LANES) / 2;
    const dim3 grid((unsigned)((n + block - 1) / block)), blk((unsigned)block);
    if (policy == 0) k_script<LdsState, NT><<<grid, blk>>>(d_blob, n, d_in, (u32)(msg_bytes / 4), d_out, (u32)out_words);
    else k_script<Lds64State, MD_SM_LANES><<<grid, blk>>>(d_blob, n, d_in, (u32)(msg_bytes / 4), d_out, (u32)out_words);
    if ((e = hipGetLastError()) != hipSuccess) break;
    *step = 5;
    if ((e = hipDeviceSynchronize()) != hipSuccess) break;
    *step = 6;
    if ((e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost)) != hipSuccess) break;
    *step = 7;
  } while (0);
  const hipError_t f1 = hipFree(d_blob), f2 = hipFree(d_in), f3 = hipFree(d_out);
  if (e != hipSuccess) return (int)e;
  if (f1 != hipSuccess) return (int)f1;
  if (f2 != hipSuccess) return (int)f2;
  return (int)f3;
}
extern "C" int md_lanes_per_block(int policy) { return (policy == 0 ? NT : MD_SM_LANES) / 2; }
extern "C" int md_stride(int policy) { return policy == 0 ? NT : MD_SM_LANES; }
