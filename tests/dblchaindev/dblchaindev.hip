// dblchaindev.hip -- TEST-ONLY device build of the arithmetic headers (fe25519.cuh, ge25519.cuh, unchanged) behind the raw-limb
// calling convention of chain_ops.cuh (fe_sq2_sub, ge_dbl_chain, ge_dbl_chain_sgn: one lane per case), and of the comb product
// ge_teeth_mul over a table in plain device memory (one lane per scalar).  Built by the Makefile next to it (run by
// tests/test_gpu_dbl_chain.py and by build()) with the product's compiler flags into tests/dblchaindev/libdblchaindev.so; the
// product never loads it.  Every case the test sends is inside the preconditions of its operation: the bound-check host program
// (tests/hostcheck/dblchaincheck.cpp) runs the same records first.
#include <hip/hip_runtime.h>
#include "chain_ops.cuh"

using namespace eg;

__global__ void k_chain_ops(int op, int n, const u32* __restrict__ in, u32* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  chain_op(op, in + (size_t)CHAIN_WORDS * i, nullptr, out + (size_t)CHAIN_WORDS * i);
}

// a lane's comb table, packed as the product packs it (device_io.cuh BaseTable: 4 x 256 bits per entry), and its Gray-walk steps
#define COMB_TABLE_WORDS (64 * 32)
#define COMB_TMP_WORDS (8 * 4 * EG_NL)
#define COMB_LANE_WORDS (COMB_TABLE_WORDS + COMB_TMP_WORDS)
struct LaneTable {
  u32* w;
  __device__ void store(int i, const ge_cached& c) {
    fe a = c.YpX, b = c.YmX, z = c.Z2;
    fe_carry(a); fe_carry(b); fe_carry(z);
    fe_pack8(w + 32 * i, a); fe_pack8(w + 32 * i + 8, b); fe_pack8(w + 32 * i + 16, z); fe_pack8(w + 32 * i + 24, c.T2d);
  }
  __device__ void load(ge_cached& c, int i) const {
    fe_unpack8(c.YpX, w + 32 * i); fe_unpack8(c.YmX, w + 32 * i + 8); fe_unpack8(c.Z2, w + 32 * i + 16); fe_unpack8(c.T2d, w + 32 * i + 24);
  }
};
struct LaneTmp {
  u32* w;
  __device__ void store(int i, const ge_cached& c) {
    for (int k = 0; k < EG_NL; ++k) {
      w[4 * EG_NL * i + k] = c.YpX.v[k]; w[4 * EG_NL * i + EG_NL + k] = c.YmX.v[k];
      w[4 * EG_NL * i + 2 * EG_NL + k] = c.Z2.v[k]; w[4 * EG_NL * i + 3 * EG_NL + k] = c.T2d.v[k];
    }
  }
  __device__ void load(ge_cached& c, int i) const {
    for (int k = 0; k < EG_NL; ++k) {
      c.YpX.v[k] = w[4 * EG_NL * i + k]; c.YmX.v[k] = w[4 * EG_NL * i + EG_NL + k];
      c.Z2.v[k] = w[4 * EG_NL * i + 2 * EG_NL + k]; c.T2d.v[k] = w[4 * EG_NL * i + 3 * EG_NL + k];
    }
  }
};

// out[i] = enc([k_i]P): every lane builds the comb table of P in its slice of `scratch` and multiplies by its own scalar
template <int T>
__global__ void k_comb(int n, const u32* __restrict__ scalars, const u32* __restrict__ point, u32* scratch, u32* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  u32 pw[8], kw[8];
  for (int j = 0; j < 8; ++j) { pw[j] = point[j]; kw[j] = scalars[8 * (size_t)i + j]; }
  ge p;
  ristretto_decode(p, pw);
  LaneTable tab{scratch + (size_t)COMB_LANE_WORDS * i};
  LaneTmp tmp{scratch + (size_t)COMB_LANE_WORDS * i + COMB_TABLE_WORDS};
  ge_teeth_tables_build<T>(tab, tmp, p);
  u64 rows[T];
  sc_recode_teeth<T>(rows, kw);
  ge acc;
  ge_teeth_mul<T>(acc, tab, rows);
  u32 o[8];
  ristretto_encode(o, acc);
  for (int j = 0; j < 8; ++j) out[8 * (size_t)i + j] = o[j];
}

// Runs a kernel over device copies of `in` (and `extra`), with `scratch_bytes` of zeroed device scratch.  Returns 0 or the first
// failing HIP status; *step says which call it came from (1 malloc, 2 copy in, 3 memset, 4 launch, 5 synchronise, 6 copy out, 7 free).
template <class Launch>
static int run_on_device(const void* in, size_t in_bytes, const void* extra, size_t extra_bytes, size_t scratch_bytes, void* out, size_t out_bytes,
                         int* step, Launch launch) {
  u32 *d_in = nullptr, *d_extra = nullptr, *d_scratch = nullptr, *d_out = nullptr;
  hipError_t e;
  *step = 1;
  do {
    if ((e = hipMalloc(&d_in, in_bytes)) != hipSuccess) break;
    if ((e = hipMalloc(&d_extra, extra_bytes ? extra_bytes : 4)) != hipSuccess) break;
    if ((e = hipMalloc(&d_scratch, scratch_bytes ? scratch_bytes : 4)) != hipSuccess) break;
    if ((e = hipMalloc(&d_out, out_bytes)) != hipSuccess) break;
    *step = 2;
    if ((e = hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    if (extra_bytes && (e = hipMemcpy(d_extra, extra, extra_bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
    *step = 3;
    if ((e = hipMemset(d_out, 0, out_bytes)) != hipSuccess) break;
    if (scratch_bytes && (e = hipMemset(d_scratch, 0, scratch_bytes)) != hipSuccess) break;
    *step = 4;
    launch(d_in, d_extra, d_scratch, d_out);
    if ((e = hipGetLastError()) != hipSuccess) break;
    *step = 5;
    if ((e = hipDeviceSynchronize()) != hipSuccess) break;
    *step = 6;
    if ((e = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost)) != hipSuccess) break;
    *step = 7;
  } while (0);
  const hipError_t f[4] = {d_in ? hipFree(d_in) : hipSuccess, d_extra ? hipFree(d_extra) : hipSuccess, d_scratch ? hipFree(d_scratch) : hipSuccess,
                           d_out ? hipFree(d_out) : hipSuccess};
  if (e != hipSuccess) return (int)e;
  for (int i = 0; i < 4; ++i) if (f[i] != hipSuccess) return (int)f[i];
  return 0;
}

extern "C" int dcd_chain_ops(int op, int n, const uint32_t* in, uint32_t* out, int block, int* step) {
  *step = 0;
  if (op < 0 || op >= COP_COUNT || n <= 0 || block < 64 || block > 256 || block % 64 != 0) return (int)hipErrorInvalidValue;
  const size_t bytes = sizeof(u32) * CHAIN_WORDS * (size_t)n;
  return run_on_device(in, bytes, nullptr, 0, 0, out, bytes, step, [&](u32* d_in, u32*, u32*, u32* d_out) {
    k_chain_ops<<<dim3((unsigned)((n + block - 1) / block)), dim3((unsigned)block)>>>(op, n, d_in, d_out);
  });
}

extern "C" int dcd_comb(int teeth, int n, const uint32_t* scalars, const uint32_t* point, uint32_t* out, int* step) {
  *step = 0;
  if ((teeth != 5 && teeth != 6) || n <= 0 || n > 4096) return (int)hipErrorInvalidValue;
  const int block = 64;
  const dim3 grid((unsigned)((n + block - 1) / block)), blk((unsigned)block);
  return run_on_device(scalars, 32 * (size_t)n, point, 32, sizeof(u32) * COMB_LANE_WORDS * (size_t)n, out, 32 * (size_t)n, step,
                       [&](u32* d_sc, u32* d_pt, u32* d_scratch, u32* d_out) {
                         if (teeth == 5) k_comb<5><<<grid, blk>>>(n, d_sc, d_pt, d_scratch, d_out);
                         else k_comb<6><<<grid, blk>>>(n, d_sc, d_pt, d_scratch, d_out);
                       });
}
extern "C" int dcd_chain_op_count() { return COP_COUNT; }
