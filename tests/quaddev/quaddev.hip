// quaddev.hip -- TEST-ONLY device build of the quad-lane point arithmetic (csrc/ge25519_quad.cuh, unchanged) behind the raw-limb cases
// of quad_ops.cuh: four adjacent lanes per case, the operation chosen by a kernel argument that is uniform over the launch.  Built by
// the Makefile next to it with the product's compiler flags into tests/quaddev/libquaddev.so; the product never loads it.
// tests/test_gpu_small_batch.py compares its raw output limbs with the bound-check host build's, which runs the same records first.
#include <hip/hip_runtime.h>
#include "quad_ops.cuh"

using namespace eg;

constexpr int QD_IN_WORDS = 8 * EG_NL;      // operands a and b, four field elements each
constexpr int QD_OUT_WORDS = 4 * EG_NL;

__global__ void k_quad_ops(int op, int n, const u32* __restrict__ in, u32* __restrict__ out) {
  const int lane = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int i = lane >> 2;
  if (i >= n) return;                        // whole quads leave together: n cases occupy 4 n lanes
  QuadDev q(lane);
  const u32* ci = in + (size_t)QD_IN_WORDS * i;
  QuadDev::var<fe> a_pt, a_cd, b_cd, res;
  const int co = quad_cached_order(q.r);
#pragma unroll
  for (int k = 0; k < EG_NL; ++k) {
    a_pt.v.v[k] = ci[q.r * EG_NL + k];
    a_cd.v.v[k] = ci[co * EG_NL + k];
    b_cd.v.v[k] = ci[(4 + co) * EG_NL + k];
  }
  bool cached;
  quad_case(q, op, a_pt, a_cd, b_cd, res, cached);
  const int oe = cached ? co : q.r;
#pragma unroll
  for (int k = 0; k < EG_NL; ++k) out[(size_t)QD_OUT_WORDS * i + oe * EG_NL + k] = res.v.v[k];
}

// Runs n cases of one operation (block: a multiple of 64, at most 256).  Returns 0 or the first failing HIP status.
extern "C" int qd_quad_ops(int op, int n, const uint32_t* in, uint32_t* out, int block) {
  if (op < 0 || op >= QOP_COUNT || n <= 0 || block < 64 || block > 256 || block % 64 != 0) return (int)hipErrorInvalidValue;
  const size_t in_bytes = sizeof(u32) * QD_IN_WORDS * (size_t)n, out_bytes = sizeof(u32) * QD_OUT_WORDS * (size_t)n;
  u32 *d_in = nullptr, *d_out = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&d_in, in_bytes)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d_out, out_bytes)) != hipSuccess) { (void)hipFree(d_in); return (int)e; }
  do {
    if ((e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    if ((e = hipMemset(d_out, 0, out_bytes)) != hipSuccess) break;
    const size_t lanes = 4 * (size_t)n;
    k_quad_ops<<<dim3((unsigned)((lanes + block - 1) / block)), dim3((unsigned)block)>>>(op, n, d_in, d_out);
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = hipDeviceSynchronize()) != hipSuccess) break;
    e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  } while (0);
  const hipError_t f1 = hipFree(d_in), f2 = hipFree(d_out);
  if (e != hipSuccess) return (int)e;
  return (int)(f1 != hipSuccess ? f1 : f2);
}
extern "C" int qd_quad_op_count() { return QOP_COUNT; }
