// dvp_fr_from_ark / dvp_fr_to_ark: Fr vectors as arkworks keeps them in memory (four LE u64 holding a 2^256 mod p, src/curve.rs:16-22)
// <-> the canonical limbs of the ABI, on the device.  What a Rust host would otherwise do per element with into_bigint() before every
// bulk call.
//
// k_fr_from_ark / k_fr_to_ark: one lane per element, two 16-byte loads, the function of fr_ark.cuh in registers (a reduction and one
// Montgomery product by a constant), two 16-byte stores.  No LDS, no scratch.  A lane reads only its own 32 bytes and both loads
// precede both stores, so either kernel may run IN PLACE (d_out == d_in): that is how dvp_prove_ark (prove.hip) turns the bytes it
// copied into the prover's witness buffer into the witness.  64 bytes of HBM traffic per element is all there is to wait for.
// This file launches nothing else, so the census knows the kernels as fr_ark.hip:k_fr_from_ark and fr_ark.hip:k_fr_to_ark.
#include <cstring>

#include "common.h"
#include "fr_ark.cuh"

namespace dvp {

__global__ void __launch_bounds__(256) k_fr_from_ark(const uint4* in, uint4* out, size_t n) {  // in and out may alias: no __restrict__
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a = in[2 * i], b = in[2 * i + 1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t r[8];
  fr_from_ark_words(w, r);
  out[2 * i] = make_uint4(r[0], r[1], r[2], r[3]);
  out[2 * i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
}

__global__ void __launch_bounds__(256) k_fr_to_ark(const uint4* in, uint4* out, size_t n) {  // in and out may alias: no __restrict__
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a = in[2 * i], b = in[2 * i + 1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t r[8];
  fr_to_ark_words(w, r);
  out[2 * i] = make_uint4(r[0], r[1], r[2], r[3]);
  out[2 * i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
}

constexpr size_t FR_ARK_MAX_N = 0xffffff00ull;  // one launch holds fewer than 2^32 threads (dvp_fr_from_be32_dev's limit)

// the argument rules of dvp_fr_from_be32_dev; d_out NULL = in place
static int ark_dev(bool to_ark, const void* d_in, size_t n, void* d_out, hipStream_t st) {
  if (!n) return DVP_OK;
  if (!d_out) d_out = const_cast<void*>(d_in);
  if (!d_in || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15) || n > FR_ARK_MAX_N) return DVP_EINVAL;
  if (to_ark)
    DVP_LAUNCH(k_fr_to_ark, dim3(cdiv(n, 256)), dim3(256), 0, st, (const uint4*)d_in, (uint4*)d_out, n);
  else
    DVP_LAUNCH(k_fr_from_ark, dim3(cdiv(n, 256)), dim3(256), 0, st, (const uint4*)d_in, (uint4*)d_out, n);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

static int ark_host_ptr(bool to_ark, const uint64_t* in, size_t n, uint64_t* out) {
  if (!n) return DVP_OK;
  if (!in || !out || n > FR_ARK_MAX_N) return DVP_EINVAL;  // before the allocation, not behind it
  DevBuf b;
  DVP_TRY(b.up(in, n * 32));  // any host alignment
  DVP_TRY(ark_dev(to_ark, b.p, n, b.p, nullptr));
  return b.down(out, n * 32);
}

}  // namespace dvp

using namespace dvp;

extern "C" int dvp_fr_from_ark_dev(const void* d_in, size_t n, void* d_out, void* stream) { return ark_dev(false, d_in, n, d_out, (hipStream_t)stream); }
extern "C" int dvp_fr_to_ark_dev(const void* d_in, size_t n, void* d_out, void* stream) { return ark_dev(true, d_in, n, d_out, (hipStream_t)stream); }
extern "C" int dvp_fr_from_ark(const uint64_t* ark, size_t n, uint64_t* out) { return ark_host_ptr(false, ark, n, out); }
extern "C" int dvp_fr_to_ark(const uint64_t* limbs, size_t n, uint64_t* out_ark) { return ark_host_ptr(true, limbs, n, out_ark); }

// the host build of the same functions, no HIP call (tests/test_fr_ark_cpu.py; tools/ark_ingest.py's "today's way")
extern "C" int dvp_debug_fr_ark_host(int to_ark, const uint64_t* in, size_t n, uint64_t* out) {
  if (!n) return DVP_OK;
  if (!in || !out) return DVP_EINVAL;
  const uint8_t* src = (const uint8_t*)in;
  uint8_t* dst = (uint8_t*)out;
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8], r[8];
    memcpy(w, src + 32 * i, 32);
    if (to_ark)
      fr_to_ark_words(w, r);
    else
      fr_from_ark_words(w, r);
    memcpy(dst + 32 * i, r, 32);
  }
  return DVP_OK;
}
extern "C" int dvp_debug_fr_ark_is_one(const uint8_t* ark) { return ark ? (fr_ark_is_one(ark) ? 1 : 0) : DVP_EINVAL; }

// dvp_msm_ctx_run on arkworks-form scalars: they are copied into the call's own device buffer and converted there, in place, on the
// stream the MSM then runs on
extern "C" int dvp_msm_ctx_run_ark(dvp_msm_ctx* c, const uint64_t* scalars_ark, size_t lo, size_t hi, uint64_t out_xy[8], int* out_is_infinity) {
  if (!c || !scalars_ark || !out_xy || !out_is_infinity || lo > hi || hi >= ((size_t)1 << 27)) return DVP_EINVAL;  // a context holds fewer than 2^27 bases
  DevBuf ds;
  MsmResult sum;
  DVP_TRY(ds.up(scalars_ark, (hi - lo) * 32));
  DVP_TRY(sum.init());
  DVP_TRY(ark_dev(false, ds.p, hi - lo, ds.p, nullptr));
  DVP_TRY(dvp_msm_ctx_run_dev(c, ds.p, lo, hi, sum.p, sum.inf(), nullptr));  // hi against the context's length: DVP_EINVAL there
  return sum.down(out_xy, out_is_infinity);
}
