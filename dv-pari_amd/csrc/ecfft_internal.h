// Internal view of the ECFFT context shared by ecfft.hip (with its stage headers ecfft_*.cuh), prove.hip and setup.hip.
#pragma once
#include <map>
#include <mutex>
#include <vector>

#include "common.h"
#include "fr.cuh"

using dvp::Fr;
using dvp::Fr29;
using dvp::Fr30;

struct MatSet {
  // twisted-butterfly constants (ecfft_twiddle.cuh): (n-1) x 2 entries each (Montgomery form, pre-sliced), layer d at offset 2*(n - (n>>d)):
  // decompose (1 / (s0 - s1), -s0), recombine (s0, s1)
  Fr30* dec = nullptr;
  Fr30* rec = nullptr;
  Fr30* win = nullptr;   // n entries: 1 / W^src(position): the input twist of an extend
  Fr30* wout = nullptr;  // n entries: W^dst(position): its output twist
};
// V and V^-1 on the 8 leaves of the stride-2^(log_n - 3) subtree, in the multiplier's constant form, + the constant 1 (k_leaf_matmul8)
struct Leaf8 {
  Fr30* enter = nullptr;  // 65 entries
  Fr30* exit = nullptr;
};
struct EnterTab {  // enter's combine tables of one stride level (k_enter_fuse_tables), h entries each
  Fr30* xe = nullptr;
  Fr30* t2 = nullptr;
};
struct ExitTab {
  Fr* xinv = nullptr;   // h
  Fr* z0inv = nullptr;  // h
  Fr* ctab = nullptr;   // sz, <Z_0^2 mod X^h> on the subtree (Montgomery)
  Fr30* fused = nullptr;  // 6 h: P | R | nA | B | B2 | XI (k_exit_fuse_tables); nullptr where the level is not folded (h == 1, or above the LDS kernels' reach)
};

struct dvp_ecfft {
  int log_n = 0;
  uint32_t n_leaves = 0;
  int device = 0;
  Fr* layers = nullptr;  // layer d at offset layer_off[d], N>>d entries, Montgomery
  std::vector<size_t> layer_off;
  std::vector<Fr> x0, t;        // per layer, Montgomery (host copies)
  // Everything below is built at its first use, under `mu`.  The entries take the lock once -- extend_inplace / extend_from,
  // ecfft_device_consts, the C ABI's enter / exit -- and everything they call (extend_io, the table builders, enter_core, exit_core and
  // the recursion between the last two) runs with it held: no path locks twice, and no table is built twice.
  std::mutex mu;
  std::map<int, MatSet> mats;   // key = sl*2 + to_even
  std::map<int, Fr*> xnn;       // key = sl ; (N>>sl) entries: leaf^((N>>sl)/2)
  std::map<int, EnterTab> enter_tabs;  // key = sl
  std::map<int, ExitTab> exit_tabs;    // key = sl
  Leaf8 leaf8;
  Fr* scratch = nullptr;        // 6 x N Fr work space for enter/exit
  Fr* d_x0 = nullptr;           // device copies of x0/t (Montgomery)
  Fr* d_t = nullptr;

  Fr* layer(int d) const { return layers + layer_off[d]; }
  ~dvp_ecfft() {  // every device allocation of the context (hipFree(nullptr) does nothing)
    for (void* p : {(void*)layers, (void*)scratch, (void*)d_x0, (void*)d_t, (void*)leaf8.enter, (void*)leaf8.exit}) (void)hipFree(p);
    for (auto& kv : mats)
      for (void* p : {(void*)kv.second.dec, (void*)kv.second.rec, (void*)kv.second.win, (void*)kv.second.wout}) (void)hipFree(p);
    for (auto& kv : xnn) (void)hipFree(kv.second);
    for (auto& kv : enter_tabs)
      for (void* p : {(void*)kv.second.xe, (void*)kv.second.t2}) (void)hipFree(p);
    for (auto& kv : exit_tabs)
      for (void* p : {(void*)kv.second.xinv, (void*)kv.second.z0inv, (void*)kv.second.ctab, (void*)kv.second.fused}) (void)hipFree(p);
  }
};


// in-place extend of `batch` vectors of (N >> sl)/2 values on the stride-2^sl subtree
int extend_inplace(dvp_ecfft* c, int sl, int to_even, dvp::Fr* data, uint32_t batch, hipStream_t st);
// out of place: `src` (batch vectors, read by the first pass only) -> `data`
int extend_from(dvp_ecfft* c, int sl, int to_even, const dvp::Fr* src, dvp::Fr* data, uint32_t batch, hipStream_t st);

namespace dvp {
// Z_0(x) = U - c0 V through the first kk isogenies (x Montgomery in, Montgomery out)
__host__ __device__ __forceinline__ Fr vanish_chain(Fr x, const Fr* __restrict__ x0s, const Fr* __restrict__ ts, int kk, Fr c0) {
  Fr u = x, v = fr_one_mont();
  for (int d = 0; d < kk; ++d) {
    Fr x0 = x0s[d], t = ts[d];
    Fr uv = fr_mul(u, v), vv = fr_sqr(v);
    Fr nu = fr_add(fr_sub(fr_sqr(u), fr_mul(x0, uv)), fr_mul(t, vv));
    Fr nv = fr_sub(uv, fr_mul(x0, vv));
    u = nu;
    v = nv;
  }
  return fr_sub(u, fr_mul(c0, v));
}

}  // namespace dvp
