// dvp_fr_from_be32: the witness as gnark's SP1 fork writes it (count x 32 bytes big-endian, unreduced) -> canonical Fr, on the device.
// gnark_element_to_fr over a vector (src/gnark_r1cs.rs:58-77,188-211; the reference runs it with into_par_iter on the host).
//
// k_fr_from_be32: one lane per element, two 16-byte loads, the reduction of fr_wire.cuh in registers, two 16-byte stores.  No LDS, no
// scratch.  A lane reads only its own 32 bytes, and both loads precede both stores, so the kernel may run IN PLACE (d_out == d_be32):
// that is how dvp_prove_be32 (prove.hip) turns the raw bytes it copied into the prover's witness buffer into the witness.
// This file launches nothing else, so the census knows the kernel as fr_wire.hip:k_fr_from_be32.
#include <cstring>

#include "common.h"
#include "fr_wire.cuh"

namespace dvp {

__global__ void __launch_bounds__(256) k_fr_from_be32(const uint4* in, uint4* out, size_t n) {  // in and out may alias: no __restrict__
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a = in[2 * i], b = in[2 * i + 1];
  const uint32_t be[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t r[8];
  fr_from_be32_words(be, r);
  out[2 * i] = make_uint4(r[0], r[1], r[2], r[3]);
  out[2 * i + 1] = make_uint4(r[4], r[5], r[6], r[7]);
}

constexpr size_t FR_WIRE_MAX_N = 0xffffff00ull;  // one launch holds fewer than 2^32 threads (the file format counts in 32 bits as well)

}  // namespace dvp

using namespace dvp;

extern "C" int dvp_fr_from_be32_dev(const void* d_be32, size_t n, void* d_out, void* stream) {
  if (!n) return DVP_OK;
  if (!d_be32 || !d_out || ((uintptr_t)d_be32 & 15) || ((uintptr_t)d_out & 15) || n > FR_WIRE_MAX_N) return DVP_EINVAL;
  DVP_LAUNCH(k_fr_from_be32, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)d_be32, (uint4*)d_out, n);
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

extern "C" int dvp_fr_from_be32(const uint8_t* be32, size_t n, uint64_t* out) {
  if (!n) return DVP_OK;
  if (!be32 || !out || n > FR_WIRE_MAX_N) return DVP_EINVAL;  // before the allocation, not behind it
  DevBuf b;
  DVP_TRY(b.up(be32, n * 32));  // any host alignment: a witness file's payload starts at byte 4
  DVP_TRY(dvp_fr_from_be32_dev(b.p, n, b.p, nullptr));
  return b.down(out, n * 32);
}

// the host build of the same function, no HIP call (tests/test_witness_wire_cpu.py)
extern "C" int dvp_debug_fr_from_be32_host(const uint8_t* be32, size_t n, uint64_t* out) {
  if (!n) return DVP_OK;
  if (!be32 || !out) return DVP_EINVAL;
  for (size_t i = 0; i < n; ++i) {
    uint32_t be[8], r[8];
    memcpy(be, be32 + 32 * i, 32);
    fr_from_be32_words(be, r);
    memcpy(out + 4 * i, r, 32);
  }
  return DVP_OK;
}
