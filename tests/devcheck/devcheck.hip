// devcheck.hip -- TEST-ONLY device build of the arithmetic headers (fe25519.cuh, ge25519.cuh, sc25519.cuh, unchanged) behind the
// raw-limb calling convention of limb_ops.cuh: one lane per case, the operation chosen by a kernel argument that is uniform over the
// launch.  Built by the Makefile next to it (run by tests/test_gpu_limb_corners.py and by build()) with the product's compiler flags
// (elastic_elgamal_amd/csrc/Makefile) into tests/devcheck/libdevcheck.so; the product never loads it.  Every case the test sends is
// inside the preconditions of its operation (tests/test_limb_corners_cpu.py runs the same records through the bound-check host
// build first).
#include <hip/hip_runtime.h>
#include "limb_ops.cuh"

using namespace eg;

// one kernel per group of operations, so that each keeps the register budget of the code it tests
template <int GROUP>
__global__ void k_limb_ops(int op, int n, const u32* __restrict__ in, u32* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const u32* ci = in + (size_t)LIMB_WORDS * i;
  u32* co = out + (size_t)LIMB_WORDS * i;
  if (GROUP == 0) limb_field_op(op, ci, nullptr, co);
  else if (GROUP == 1) limb_canon_op(op, ci, nullptr, co);
  else if (GROUP == 2) limb_chain_op(op, ci, nullptr, co);
  else if (GROUP == 3) limb_p1p1_op(op, ci, nullptr, co);
  else if (GROUP == 4) limb_point_op(op, ci, nullptr, co);
  else limb_scalar_op(op, ci, co);
}

// Runs n cases of one operation with the given block size (a multiple of 64, at most 256).  Returns 0 or the first failing HIP
// status; *step says which call it came from (1 malloc, 2 copy in, 3 memset, 4 launch, 5 synchronise, 6 copy out, 7 free).
extern "C" int dc_limb_ops(int op, int n, const uint32_t* in, uint32_t* out, int block, int* step) {
  *step = 0;
  if (op < 0 || op >= LOP_COUNT || n <= 0 || block < 64 || block > 256 || block % 64 != 0) return (int)hipErrorInvalidValue;
  const size_t bytes = sizeof(u32) * LIMB_WORDS * (size_t)n;
  u32 *d_in = nullptr, *d_out = nullptr;
  hipError_t e;
  *step = 1;
  if ((e = hipMalloc(&d_in, bytes)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&d_out, bytes)) != hipSuccess) { (void)hipFree(d_in); return (int)e; }
  do {
    *step = 2;
    if ((e = hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    *step = 3;
    if ((e = hipMemset(d_out, 0, bytes)) != hipSuccess) break;
    *step = 4;
    const dim3 grid((unsigned)((n + block - 1) / block)), blk((unsigned)block);
    switch (limb_op_group(op)) {
      case 0: k_limb_ops<0><<<grid, blk>>>(op, n, d_in, d_out); break;
      case 1: k_limb_ops<1><<<grid, blk>>>(op, n, d_in, d_out); break;
      case 2: k_limb_ops<2><<<grid, blk>>>(op, n, d_in, d_out); break;
      case 3: k_limb_ops<3><<<grid, blk>>>(op, n, d_in, d_out); break;
      case 4: k_limb_ops<4><<<grid, blk>>>(op, n, d_in, d_out); break;
      default: k_limb_ops<5><<<grid, blk>>>(op, n, d_in, d_out); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) break;
    *step = 5;
    if ((e = hipDeviceSynchronize()) != hipSuccess) break;
    *step = 6;
    if ((e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost)) != hipSuccess) break;
    *step = 7;
  } while (0);
  const hipError_t f1 = hipFree(d_in), f2 = hipFree(d_out);
  if (e != hipSuccess) return (int)e;
  if (f1 != hipSuccess) return (int)f1;
  return (int)f2;
}
extern "C" int dc_limb_op_count() { return LOP_COUNT; }
