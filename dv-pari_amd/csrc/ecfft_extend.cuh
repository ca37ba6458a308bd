// ECFFT, stage 5: one extend as a sequence of launches (extend_io) and its entries extend_inplace / extend_from.
// Part of ecfft.hip's translation unit: host code at global scope behind `using namespace dvp`.
#pragma once
#include <type_traits>
#include "ecfft_lds.cuh"
#include "ecfft_twiddle.cuh"

// host-side description of an extend's folded-in pointwise stages (ExtIo, ecfft_lds.cuh; SM is picked at run time)
struct ExtIoSpec {
  int sm = 0;
  const Fr30* pre = nullptr;   // replaces the input twist (a table that already contains it)
  int lshift = 0;
  const Fr30* post = nullptr;  // replaces the output twist
  Fr* out = nullptr;
  const Fr30* tb = nullptr;
  const Fr30* tc = nullptr;
  const Fr* aux = nullptr;
  int ashift = 0, aoff = 0, lh = 0;
};
constexpr int EXT_TOP_MAX = 9;  // == FUSE_LOG - 2 (asserted in extend_io): the layers one k_extend_top launch covers
// can an extend of vectors of n values carry an ExtIoSpec?  Its first and last launch must be the LDS kernels (k_extend_top /
// k_extend_fused): 2 <= n <= 2^(FUSE_LOG + EXT_TOP_MAX); the combine (sm 3) pairs two vectors inside one k_extend_fused block
// (sm 3 inside one k_extend_fused block: n <= 1024; across the two vectors of a k_extend_top tile: n >= 4096.  n = 2048 -- one
// vector per k_extend_fused block, no top -- keeps the separate k_enter_combine)
static bool ext_io_ok(uint32_t n, int sm) { return n >= 2 && n <= (1u << (11 + EXT_TOP_MAX)) && (sm != 3 || n != 2048u); }

// a run-time value as a compile-time constant for f: the BATCH of a register pass (2, 3, 4; anything else runs as one long vector: 1) ...
template <class F>
static void with_batch(uint32_t batch, F&& f) {
  switch (batch) {
    case 4: return f(std::integral_constant<int, 4>());
    case 3: return f(std::integral_constant<int, 3>());
    case 2: return f(std::integral_constant<int, 2>());
    default: return f(std::integral_constant<int, 1>());
  }
}
// ... and the store form SM of an LDS kernel's ExtIo (0 .. 3)
template <class F>
static void with_sm(int sm, F&& f) {
  switch (sm) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 0>());
  }
}

// extend of `batch` vectors of n = (N>>sl)/2 values, `src_in` -> `data` (the same buffer, or one the first launch alone reads), with
// the caller's pointwise stages folded into its first / last launch when `io` is set.  The caller holds c->mu.
static int extend_io(dvp_ecfft* c, int sl, int to_even, const Fr* src_in, Fr* data, uint32_t batch, hipStream_t st, const ExtIoSpec* io) {
  uint32_t n = (c->n_leaves >> sl) >> 1;
  if (io && !ext_io_ok(n, io->sm)) return DVP_EINVAL;
  if (n <= 1) {
    if (src_in != data && n == 1) DVP_HIP(hipMemcpyAsync(data, src_in, (size_t)batch * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return DVP_OK;
  }
  const Fr* src = src_in;  // becomes `data` after the first launch
  MatSet* ms;
  DVP_TRY(build_matset(c, sl, to_even, &ms, st));
  int ln = 31 - __builtin_clz(n);
  // The first launch multiplies its input by the source twist, the last one its output by the destination twist (see "TWISTED
  // butterflies", ecfft_twiddle.cuh); a pass knows which it is from `first` / the `last` flag of its caller.
  bool first = true;
  auto pre_of = [&]() { const Fr30* r = first ? (io && io->pre ? io->pre : ms->win) : nullptr; first = false; return r; };
  const Fr30* wout = io && io->post ? io->post : ms->wout;
  const int sm_last = io ? io->sm : 0;
  // the ExtIo of one LDS-kernel launch: `pre` set = it is the first one (and reads with the caller's stride), `last` = it carries the
  // output side (twist alone, or the caller's folded-in store)
  auto fill = [&](auto& e, const Fr30* pre, bool last) {
    e.pre = pre;
    e.lshift = pre && io ? io->lshift : 0;
    if (last) {
      e.post = wout;
      if (io) {
        e.out = io->out; e.tb = io->tb; e.tc = io->tc; e.aux = io->aux; e.ashift = io->ashift; e.aoff = io->aoff; e.lh = io->lh;
      }
    }
  };
  // one register pass over the g = 1, 2 or 3 layers d (the widest) .. d + g - 1 (k_butterfly, k_butterfly4, k_butterfly8); DEC =
  // std::true_type: decompose.  Blocks are contiguous, so `batch` vectors of n behave like one vector of batch * n for the block structure;
  // the BATCH template only buys constant reuse when the batch is small and n is large: 2 .. 4 vectors run side by side over n (a lane
  // per vector from two layers per pass up, a loop inside k_butterfly), anything else as one long vector
  auto pass = [&](auto DEC, int d, int g, bool last) {
    constexpr bool dec = decltype(DEC)::value;
    auto tw = [&](int k) { return (dec ? ms->dec : ms->rec) + 2 * (size_t)(n - (n >> (d + k))); };  // layer d + k
    const int lh = ln - d - g;  // log2 of the narrowest layer's pair distance
    const Fr30* pre = pre_of();
    const Fr30* post = last ? wout : nullptr;
    const bool side = batch >= 2 && batch <= 4;
    const uint32_t nn = side ? n : (uint32_t)((size_t)batch * n);
    const dim3 grid(cdiv((size_t)(nn >> g) * (side && g > 1 ? batch : 1), TPB)), blk(TPB);
    with_batch(batch, [&](auto B) {
      constexpr int b = decltype(B)::value;
      if (g == 1) DVP_LAUNCH((k_butterfly<b, dec>), grid, blk, 0, st, src, data, tw(0), lh, nn, pre, post, n);
      else if (g == 2) DVP_LAUNCH((k_butterfly4<b, dec>), grid, blk, 0, st, src, data, tw(0), tw(1), lh, nn, pre, post, n);
      else DVP_LAUNCH((k_butterfly8<b, dec>), grid, blk, 0, st, src, data, tw(0), tw(1), tw(2), lh, nn, pre, post, n);
    });
    src = data;
  };
  const int lb = ln < FUSE_LOG ? ln : FUSE_LOG;  // layers handled inside LDS
  const int top = ln - lb;
  // the top layers in groups of 3 (radix 8), then one group of 2 or 1; the recombine direction mirrors the decompose's grouping
  const int radix = (int)tune().ecfft_radix4;  // 0: one layer per pass, 1: two, 2: three, 3 (default): the top in one LDS-tiled launch
  // k_extend_top covers the last tl <= TOP_MAX top layers (the ones next to the fused bottom), whatever is above them goes in groups
  constexpr int TOP_MAX = FUSE_LOG - 2;  // >= 4 columns per tile row (128-byte lines); below 4 layers k_butterfly8 / 4 do as well
  static_assert(TOP_MAX == EXT_TOP_MAX && FUSE_LOG == 11, "ext_io_ok restates these");
  const int TOP_MIN = io ? 1 : 4;        // an extend with folded-in stages needs its first and last launch to be LDS kernels
  const int tl = ((radix >= 3 || io) && top >= TOP_MIN) ? (top < TOP_MAX ? top : TOP_MAX) : 0;
  const int d0 = top - tl;  // layers 0 .. d0 - 1 in groups, d0 .. top - 1 tiled
  // the decompose side is never the last launch (SM 0); on the recombine side the first launch is long past (pre_of() gives nullptr)
  auto pass_top = [&](auto DEC, bool last) {
    constexpr bool dec = decltype(DEC)::value;
    const uint32_t nn = (uint32_t)((size_t)batch * n);  // the batch vectors are contiguous: blocks of n >> d0 values all the way through
    const dim3 g(nn >> FUSE_LOG), b(FUSE_TPB);
    const Fr30* pre = pre_of();
    auto go = [&](auto SM) {
      ExtIo<decltype(SM)::value> e;
      fill(e, pre, last);
      DVP_LAUNCH((k_extend_top<dec, decltype(SM)::value>), g, b, 0, st, src, data, dec ? ms->dec : ms->rec, n, ln, d0, tl, batch, e);
    };
    if constexpr (dec) go(std::integral_constant<int, 0>()); else with_sm(last ? sm_last : 0, go);
    src = data;
  };
  std::vector<int> groups;
  for (int left = d0; left > 0;) {
    const int g = radix >= 2 && left >= 3 ? 3 : (radix >= 1 && left >= 2 ? 2 : 1);
    groups.push_back(g);
    left -= g;
  }
  {
    int d = 0;
    for (int g : groups) {
      pass(std::true_type(), d, g, false);
      d += g;
    }
    if (tl) pass_top(std::true_type(), false);
  }
  {
    const size_t total = (size_t)batch * n;
    const Fr30* pre = pre_of();
    const bool last = top == 0;
    with_sm(last ? sm_last : 0, [&](auto SM) {
      ExtIo<decltype(SM)::value> e;
      fill(e, pre, last);
      DVP_LAUNCH((k_extend_fused<decltype(SM)::value>), dim3(cdiv(total, FUSE_ELEMS)), dim3(FUSE_TPB), 0, st, src, data, ms->dec, ms->rec, n, ln, lb, total, e);
    });
    src = data;
  }
  {
    if (tl) pass_top(std::false_type(), d0 == 0);
    int d = d0;
    for (size_t k = groups.size(); k-- > 0;) {
      d -= groups[k];
      pass(std::false_type(), d, groups[k], d == 0);
    }
  }
  DVP_HIP(hipGetLastError());
  return DVP_OK;
}

// The entries of prove.hip, setup.hip and the C ABI (ecfft_internal.h); they take the context's lock.
// in-place extend of `batch` vectors of n = (N>>sl)/2 values
int extend_inplace(dvp_ecfft* c, int sl, int to_even, Fr* data, uint32_t batch, hipStream_t st) { return extend_from(c, sl, to_even, data, data, batch, st); }
// the same out of place: `src` is read by the first pass only and left untouched (the prover keeps a, b, c on D for its K scalars;
// a copy of 3 x 32 MB before every extend was one more HBM round trip)
int extend_from(dvp_ecfft* c, int sl, int to_even, const Fr* src_in, Fr* data, uint32_t batch, hipStream_t st) {
  std::lock_guard<std::mutex> g(c->mu);
  return extend_io(c, sl, to_even, src_in, data, batch, st, nullptr);
}
