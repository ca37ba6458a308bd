// ECFFT: read-outs for the parity tests and the FFTR tree files -- a layer of the domain, and the butterfly matrices the reference keeps.
// Part of ecfft.hip's translation unit: host code at global scope behind `using namespace dvp`.
#pragma once
#include "ecfft_enter_exit.cuh"

// Parity-test read-out of the butterfly matrices extend() runs on (include/dvpari_internal.h): what the reference keeps
// in FFTree::{decompose,recombine}_matrices and stores in sections 2 / 1 of its FFTR tree files (src/tree_io.rs:353-433).
namespace dvp {
__global__ void __launch_bounds__(256) k_mats_export(const Fr29* __restrict__ in, Fr* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t l[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) l[k] = in[i].l[k];
  out[i] = fr_from_mont(fr_from29(l));
}
}  // namespace dvp
extern "C" int dvp_debug_ecfft_matrices(dvp_ecfft* c, int to_even, int which, uint64_t* out) {
  if (!c || !out || (to_even != 0 && to_even != 1) || (which != 0 && which != 1) || c->log_n < 2) return DVP_EINVAL;
  // the TRUE 2x2 matrices (what the reference stores), rebuilt on demand: extend() itself runs on the twisted constants
  const uint32_t nv = c->n_leaves >> 1;
  const size_t n = ((size_t)nv - 1) * 4;
  DevBuf dec, rec, tmp;
  DVP_TRY(dec.alloc(n * sizeof(Fr29)));
  DVP_TRY(rec.alloc(n * sizeof(Fr29)));
  DVP_TRY(tmp.alloc(n * sizeof(Fr)));
  const int src = to_even ? 1 : 0, dst = to_even ? 0 : 1;
  const int ln = 31 - __builtin_clz(nv);
  for (int d = 0; d < ln; ++d) {
    const uint32_t nd = nv >> d;
    const size_t off = 4 * (size_t)(nv - nd);
    DVP_LAUNCH(k_build_mats, dim3(cdiv(nd >> 1, TPB)), dim3(TPB), 0, 0, c->layer(d), 0, nd, c->x0[d], src, dst, dec.as<Fr29>() + off,
                       rec.as<Fr29>() + off);
  }
  DVP_LAUNCH(k_mats_export, dim3(cdiv(n, TPB)), dim3(TPB), 0, 0, which ? rec.as<Fr29>() : dec.as<Fr29>(), tmp.as<Fr>(), n);
  DVP_HIP(hipGetLastError());
  return tmp.down(out, n * sizeof(Fr));
}
// layer d (N >> d values), out of Montgomery form, to the host (dvp_ecfft_leaves: d = 0)
static int layer_to_host(const dvp_ecfft* c, uint32_t d, uint64_t* out) {
  if (!c || !out || d > (uint32_t)c->log_n) return DVP_EINVAL;
  const size_t n = c->n_leaves >> d;
  DevBuf tmp;
  DVP_TRY(tmp.alloc(n * sizeof(Fr)));
  DVP_LAUNCH(k_from_mont, dim3(cdiv(n, TPB)), dim3(TPB), 0, 0, c->layer((int)d), tmp.as<Fr>(), n);
  DVP_HIP(hipGetLastError());
  return tmp.down(out, n * sizeof(Fr));
}
extern "C" int dvp_debug_ecfft_layer(const dvp_ecfft* c, uint32_t d, uint64_t* out) { return layer_to_host(c, d, out); }
