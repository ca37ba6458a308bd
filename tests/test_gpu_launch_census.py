"""GPU path tests (-m gpu): which kernel variants a knob or a size really selects, beside the oracle comparison.

msm_core, the ECFFT and k_batch_inverse choose between some 140 kernels and template variants by ~40 DVP_* knobs and by sizes only
the device knows; a dispatch that falls back to the general kernel still returns the right point.  The library counts every launch
per variant (csrc/common.h: the launch census), and every row below says four things: the input, the knobs, the variants that must
have run and the variants that must not.  A row resets the profile, runs once, compares the result with the oracle -- k233_mulgen
of the scalar-log dot product for an MSM, c_oracle.FFTree / Python integers element for element otherwise -- and only then reads
the census.  test_every_variant_runs runs the whole table behind one reset and demands a launch of every variant of msm.hip,
ecfft.hip and fr_ops.hip that is no diagnostic.

What selects what (msm.hip: msm_core; n = points, W = windows, nk = buckets, e = n W entries):
  * pair rounds planned: ra_plan = the r with (e >> r) >= DVP_MSM_AFF_MIN > (e >> (r + 1)); run: as many as the largest bucket needs;
  * all-rounds bookkeeping (k_mscan_*, k_round_desc_all) when DVP_MSM_ROUND_PIPELINE != 0, ra_plan >= 2 and e >= 4 nk, otherwise
    k_post_sort and per-round k_round_desc; descriptor lanes per bucket 64 / 16 / 4 by (e >> (r + 1)) / nk >= 48 / >= 8 / below;
  * what the rounds leave: at most one point per bucket -> k_bucket_gather_items (no round) / k_bucket_gather_aff; at most
    DVP_MSM_BUCKET_PAIRS_MAX per bucket after a round -> k_bucket_pairs + k_bucket_rest; else the fan-in-K reducer, first level
    k_accum_affine_fast + _rest (DVP_MSM_ACCUM_FAST) or k_accum_affine, <INDIRECT = no round ran, QUAD = tasks' bound <=
    DVP_MSM_ACCUM_QUAD_MAX>, further levels k_accum_proj<16 / 4 / 1>.
The exceptional input (eight points and their negatives) fills its buckets with equal and opposite points; one pair round turns
them into doublings and infinity markers, and after four the survivors are sums of sixteen and practically never collide: the rest
list is non-empty when the rounds stop after none or one (DVP_MSM_AFF_MIN = 2^19 / 2^15), which is where the rows demand it."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import c_oracle as co
import ecfft_cases as ec
import pyref as o
import msm_cases as mc
from util import to_limbs, from_limbs, np_to_pt, rand_fr_np

pytestmark = pytest.mark.gpu
BIG = 1 << 30
M = "msm.hip:"


def fam(prefix, *names):
    return [prefix + n for n in names]


F_RECODE = fam(M, "k_recode<unsigned short>", "k_recode<unsigned int>", "k_recode_signed")
F_SORT1 = fam(M, "k_hist_local", "k_hist_scan", "k_scatter_local")
F_SORT2 = fam(M, "k_hist_local2", "k_hist_scan2", "k_part_scan_chunks", "k_part_scan_totals", "k_part_starts")
F_LEVEL1 = fam(M, "k_part_hist_signed", "k_part_hist")
F_SCATTER1 = fam(M, "k_part_scatter_signed<true>", "k_part_scatter_signed<false>", "k_part_scatter_staged", "k_part_scatter")
F_SCATTER2 = fam(M, "k_scatter_local2_staged", "k_scatter_local2")
F_BOOK = fam(M, "k_post_sort", "k_mscan_local", "k_mscan_bsums", "k_mscan_add")
F_DESC = fam(M, "k_round_desc<4>", "k_round_desc<16>", "k_round_desc<64>", "k_round_desc_all<4,false>", "k_round_desc_all<16,false>",
             "k_round_desc_all<64,false>", "k_round_desc_all<4,true>", "k_round_desc_all<16,true>", "k_round_desc_all<64,true>")
F_ROUND = fam(M, "k_affine_round<true,false,false>", "k_affine_round<false,false,false>", "k_affine_round<false,false,true>",
              "k_affine_round<true,true,false>", "k_affine_round<false,true,false>", "k_affine_round<false,true,true>")
F_FIRST = fam(M, "k_bucket_gather_items", "k_bucket_gather_aff", "k_bucket_pairs", "k_bucket_rest",
              "k_accum_affine<true,true>", "k_accum_affine<true,false>", "k_accum_affine<false,true>", "k_accum_affine<false,false>",
              "k_accum_affine_fast<true,true>", "k_accum_affine_fast<true,false>", "k_accum_affine_fast<false,true>",
              "k_accum_affine_fast<false,false>", "k_accum_affine_rest<true>", "k_accum_affine_rest<false>")
F_PROJ = fam(M, "k_accum_proj<1>", "k_accum_proj<4>", "k_accum_proj<16>")
F_MERGE = fam(M, "k_merge<1,true>", "k_merge<1,false>", "k_merge<4,true>", "k_merge<4,false>", "k_merge<16,true>", "k_merge<16,false>")
F_TAIL = fam(M, "k_tail<true>", "k_tail<false>", "k_tail_groups")
F_TABLE = fam(M, "k_dbl_table", "k_frob_table")
F_SCAN = fam(M, "k_scan_add_fold", "k_scan_bsums", "k_scan_add")

ROUND0, LATER_WORD, LATER_DENSE = "k_affine_round<true,false,false>", "k_affine_round<false,false,false>", "k_affine_round<false,false,true>"
# the sort of a one-shot MSM (per-window bucket sets, 16-bit digits, one level) and of the default fixed-base flavour (signed windows,
# level 1 recomputes the entry words: nothing is recoded to HBM)
ONE_SHOT = [(F_RECODE, ["k_recode<unsigned short>"]), (F_SORT1, "all"), (F_SORT2 + F_LEVEL1 + F_SCATTER1 + F_SCATTER2, []), (F_TABLE, [])]
FIXED = [(F_SORT1, []), (F_SORT2, "all")]
SIGNED = FIXED + [(F_RECODE, []), (F_LEVEL1, ["k_part_hist_signed"])]
NO_ROUNDS = [(F_ROUND, []), (F_DESC, []), (F_BOOK, ["k_post_sort"])]


class Row:
    """input name, route ("os": one-shot, "fx": a fixed-base context made under `ctx`), knobs of the run, paths = [(family, the
    members that run; the others must not)], rest = None / ">0" / "==0": the rest list's length after the run"""

    def __init__(self, rid, inp, route, knobs, paths, rest=None, ctx=None, table=False):
        self.id, self.inp, self.route, self.knobs, self.rest, self.ctx, self.table = rid, inp, route, dict(knobs), rest, dict(ctx or {}), table
        self.ran, self.idle = [], []
        for family, members in paths:
            members = family if members == "all" else [m if ":" in m else M + m for m in members]
            assert set(members) <= set(family), (rid, set(members) - set(family))
            self.ran += members
            self.idle += [x for x in family if x not in members]


def reducer(first, proj=None):
    return [(F_FIRST, first)] + ([(F_PROJ, proj)] if proj is not None else [])


RA0 = dict(DVP_MSM_AFF_MIN=1 << 19)     # no pair round at these sizes (e <= 6000 x 30)
ONE_ROUND = dict(DVP_MSM_AFF_MIN=1 << 15)  # e = 4096 x 22 or x 30: e / 2 >= 2^15 > e / 4, one round planned; no all-rounds bookkeeping (ra_plan < 2)
AFTER_ONE = [(F_ROUND, [ROUND0]), (F_DESC, []), (F_BOOK, ["k_post_sort"])]
LANE, QUAD = dict(DVP_MSM_ACCUM_QUAD_MAX=1), dict(DVP_MSM_ACCUM_QUAD_MAX=BIG)
FX11, FX8, FX13 = dict(DVP_MSM_FIXED_C=11), dict(DVP_MSM_FIXED_C=8), dict(DVP_MSM_FIXED_C=13)

MSM_ROWS = [
    # ---- one-shot, c = 11: nk = 23 x 2048 buckets, so a reducer level's task bound (> nk) exceeds ACCUM_HEX_MAX = 32768: no k_accum_proj<16>
    Row("os-ra0-fast-lane", "X", "os", dict(DVP_MSM_C=11, **RA0, **LANE), ONE_SHOT + NO_ROUNDS +
        reducer(["k_accum_affine_fast<true,false>", "k_accum_affine_rest<true>"], ["k_accum_proj<1>"]) + [(F_TAIL, ["k_tail_groups", "k_tail<false>"])], rest=">0"),
    Row("os-ra0-fast-quad", "X", "os", dict(DVP_MSM_C=11, **RA0, **QUAD), ONE_SHOT + NO_ROUNDS +
        reducer(["k_accum_affine_fast<true,true>", "k_accum_affine_rest<true>"], ["k_accum_proj<4>"]), rest=">0"),
    Row("os-ra0-general-lane", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_ACCUM_FAST=0, **RA0, **LANE), ONE_SHOT + NO_ROUNDS + reducer(["k_accum_affine<true,false>"], ["k_accum_proj<1>"]), rest="==0"),
    Row("os-ra0-general-quad", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_ACCUM_FAST=0, **RA0, **QUAD), ONE_SHOT + NO_ROUNDS + reducer(["k_accum_affine<true,true>"], ["k_accum_proj<4>"]), rest="==0"),
    # the default of a small one-shot MSM: 3 000 random points, nothing set but the window (tasks' bound 76 k > ACCUM_QUAD_MAX = 49 152)
    Row("os-default-random", "R3", "os", dict(DVP_MSM_C=11), ONE_SHOT + NO_ROUNDS + reducer(["k_accum_affine_fast<true,false>", "k_accum_affine_rest<true>"], ["k_accum_proj<1>"]) +
        [(F_SCAN, ["k_scan_add_fold"])], rest="==0"),
    Row("os-round1-fast-lane", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=0, **ONE_ROUND, **LANE), ONE_SHOT + AFTER_ONE +
        reducer(["k_accum_affine_fast<false,false>", "k_accum_affine_rest<false>"]), rest=">0"),
    Row("os-round1-fast-quad", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=0, **ONE_ROUND, **QUAD), ONE_SHOT + AFTER_ONE +
        reducer(["k_accum_affine_fast<false,true>", "k_accum_affine_rest<false>"]), rest=">0"),
    Row("os-round1-general-lane", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_ACCUM_FAST=0, **ONE_ROUND, **LANE), ONE_SHOT + AFTER_ONE + reducer(["k_accum_affine<false,false>"]), rest="==0"),
    Row("os-round1-general-quad", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=0, DVP_MSM_ACCUM_FAST=0, **ONE_ROUND, **QUAD), ONE_SHOT + AFTER_ONE + reducer(["k_accum_affine<false,true>"]), rest="==0"),
    # ~400 points per bucket after the one round: only DVP_MSM_BUCKET_PAIRS_MAX = 100000 sends them to k_bucket_pairs; with 12 the reducer takes them
    Row("os-round1-pairs", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=100000, **ONE_ROUND), ONE_SHOT + AFTER_ONE + reducer(["k_bucket_pairs", "k_bucket_rest"], []), rest=">0"),
    Row("os-round1-pairs-max-12", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_BUCKET_PAIRS_MAX=12, **ONE_ROUND, **LANE), ONE_SHOT + AFTER_ONE +
        reducer(["k_accum_affine_fast<false,false>", "k_accum_affine_rest<false>"]), rest=">0"),
    # 3 000 random points, c = 8: e = 90 000 over nk = 31 x 256, four rounds planned (e >> 4 >= 4096 > e >> 5) and e >= 4 nk: the all-rounds
    # bookkeeping with 4 lanes per bucket ((e >> 2) / nk = 2); buckets of ~11 points leave one or two each
    Row("os-pairs-random", "R3", "os", dict(DVP_MSM_C=8, DVP_MSM_AFF_MIN=4096, DVP_MSM_BUCKET_PAIRS_MAX=12), ONE_SHOT +
        [(F_BOOK, ["k_mscan_local", "k_mscan_bsums", "k_mscan_add"]), (F_DESC, ["k_round_desc_all<4,false>"]), (F_ROUND, [ROUND0, LATER_WORD])] +
        reducer(["k_bucket_pairs", "k_bucket_rest"], []), rest="==0"),
    # one point (a one-shot MSM's windows are tau-adic: only a lone point is sure to be alone in every bucket): no round, nothing to add
    # before the merge tree
    Row("os-singletons", "ONE", "os", dict(DVP_MSM_C=11), ONE_SHOT + NO_ROUNDS + reducer(["k_bucket_gather_items"], [])),
    # rounds to the bottom: e = 90 112 < 4 nk keeps the per-round bookkeeping, (e >> (r + 1)) / nk < 8: 4 lanes per bucket
    Row("os-rounds-to-bottom", "X", "os", dict(DVP_MSM_C=11, DVP_MSM_AFF_MIN=32), ONE_SHOT + [(F_BOOK, ["k_post_sort"]), (F_DESC, ["k_round_desc<4>"]), (F_ROUND, [ROUND0, LATER_WORD])] +
        reducer(["k_bucket_gather_aff"], [])),
    Row("os-proj-mode-lane", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_PROJ=1, DVP_MSM_AFF_MIN=32, DVP_MSM_K=2, DVP_MSM_ACCUM_HEX_MAX=0, **LANE), ONE_SHOT + NO_ROUNDS +
        reducer(["k_accum_affine_fast<true,false>", "k_accum_affine_rest<true>"], ["k_accum_proj<1>"])),
    Row("os-proj-mode-quad", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_PROJ=1, DVP_MSM_AFF_MIN=32, DVP_MSM_K=2, DVP_MSM_ACCUM_HEX_MAX=0, **QUAD), ONE_SHOT + NO_ROUNDS +
        reducer(["k_accum_affine_fast<true,true>", "k_accum_affine_rest<true>"], ["k_accum_proj<4>"])),
    # merge tree and tail of the one-shot flavour (levels of (nk >> (j + 1)) (j + 1) additions, at least 253 here)
    Row("os-merge-quads", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=BIG), ONE_SHOT + [(F_MERGE, ["k_merge<4,true>", "k_merge<4,false>"])]),
    Row("os-merge-lanes", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=1), ONE_SHOT + [(F_MERGE, ["k_merge<1,true>", "k_merge<1,false>"])]),
    Row("os-merge-rows", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_HEX_MAX=BIG), ONE_SHOT + [(F_MERGE, ["k_merge<16,true>", "k_merge<16,false>"])]),
    Row("os-tail-single", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_TAIL_GROUPS=0), ONE_SHOT + [(F_TAIL, ["k_tail<false>"])]),
    Row("os-tail-groups", "R3", "os", dict(DVP_MSM_C=11, DVP_MSM_TAIL_GROUPS=1), ONE_SHOT + [(F_TAIL, ["k_tail_groups", "k_tail<false>"])]),
    # ---- fixed-base tables and recodes
    Row("fx-table-signed", "R6", "fx", {}, SIGNED + [(F_TABLE, ["k_dbl_table"]), (F_TAIL, ["k_tail<true>"])], ctx=dict(DVP_MSM_ALIGNED_SIGNED=1, **FX11), table=True),
    Row("fx-table-tau", "R6", "fx", {}, FIXED + [(F_TABLE, ["k_frob_table"]), (F_RECODE, ["k_recode<unsigned int>"]), (F_LEVEL1, ["k_part_hist"]), (F_TAIL, ["k_tail<false>"])],
        ctx=dict(DVP_MSM_ALIGNED_SIGNED=0, **FX11), table=True),
    Row("fx-recode-to-hbm", "R6", "fx", dict(DVP_MSM_SORT_FUSED=0), FIXED + [(F_RECODE, ["k_recode_signed"]), (F_LEVEL1, ["k_part_hist"]), (F_SCATTER1, ["k_part_scatter"])], ctx=FX8),
    # ---- the two-level sort's scatters: level 1 staged from 64 partitions up (DVP_FX_HI >= 6), level 2 staged up to 10 low bits
    Row("fx-sort-c20-fused", "R6", "fx", {}, SIGNED + [(F_SCATTER1, ["k_part_scatter_signed<true>"]), (F_SCATTER2, ["k_scatter_local2_staged"]), (F_SCAN, ["k_scan_bsums", "k_scan_add"])],
        ctx=dict(DVP_MSM_FIXED_C=20)),
    Row("fx-sort-c20-unfused", "R6", "fx", dict(DVP_MSM_SORT_FUSED=0), FIXED + [(F_RECODE, ["k_recode_signed"]), (F_LEVEL1, ["k_part_hist"]), (F_SCATTER1, ["k_part_scatter_staged"]),
                                                                                   (F_SCATTER2, ["k_scatter_local2_staged"])], ctx=dict(DVP_MSM_FIXED_C=20)),
    Row("fx-sort-plain-scatters", "R6", "fx", {}, SIGNED + [(F_SCATTER1, ["k_part_scatter_signed<false>"]), (F_SCATTER2, ["k_scatter_local2"])], ctx=dict(DVP_MSM_FIXED_C=18, DVP_FX_HI=2)),
    Row("fx-sort-plain-unfused", "R6", "fx", dict(DVP_MSM_SORT_FUSED=0), FIXED + [(F_LEVEL1, ["k_part_hist"]), (F_SCATTER1, ["k_part_scatter"]), (F_SCATTER2, ["k_scatter_local2"])],
        ctx=dict(DVP_MSM_FIXED_C=18, DVP_FX_HI=2)),
    Row("fx-sort-tau-staged", "R6", "fx", {}, FIXED + [(F_RECODE, ["k_recode<unsigned int>"]), (F_LEVEL1, ["k_part_hist"]), (F_SCATTER1, ["k_part_scatter_staged"])],
        ctx=dict(DVP_MSM_FIXED_C=20, DVP_MSM_ALIGNED_SIGNED=0)),
    # ---- round bookkeeping: 6 000 points, rounds to the bottom; c = 8 / 11 / 13: e = 180 000 / 132 000 / 108 000 over nk = 128 / 1 024 / 4 096
    Row("fx-book-per-round", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_PIPELINE=0, DVP_MSM_ROUND_DENSE=1), SIGNED +
        [(F_BOOK, ["k_post_sort"]), (F_DESC, ["k_round_desc<64>", "k_round_desc<16>", "k_round_desc<4>"]), (F_ROUND, [ROUND0, LATER_WORD])] + reducer(["k_bucket_gather_aff"], []), ctx=FX8),
    Row("fx-book-all-64-word", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_PIPELINE=2, DVP_MSM_ROUND_DENSE=0), SIGNED +
        [(F_BOOK, ["k_mscan_local", "k_mscan_bsums", "k_mscan_add"]), (F_DESC, ["k_round_desc_all<64,false>"]), (F_ROUND, [ROUND0, LATER_WORD])], ctx=FX8),
    Row("fx-book-all-64-dense", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_PIPELINE=2, DVP_MSM_ROUND_DENSE=1), SIGNED +
        [(F_BOOK, ["k_mscan_local", "k_mscan_bsums", "k_mscan_add"]), (F_DESC, ["k_round_desc_all<64,true>"]), (F_ROUND, [ROUND0, LATER_DENSE])], ctx=FX8),
    # (the side stream keeps the sort's own scan and k_post_sort beside the all-rounds scan)
    Row("fx-book-side-stream", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_PIPELINE=1, DVP_MSM_ROUND_DENSE=1), SIGNED +
        [(F_BOOK, "all"), (F_DESC, ["k_round_desc_all<64,true>"]), (F_ROUND, [ROUND0, LATER_DENSE])], ctx=FX8),
    Row("fx-book-all-16-word", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_DENSE=0), SIGNED + [(F_DESC, ["k_round_desc_all<16,false>"]), (F_ROUND, [ROUND0, LATER_WORD])], ctx=FX11),
    Row("fx-book-all-16-dense", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_DENSE=1), SIGNED + [(F_DESC, ["k_round_desc_all<16,true>"]), (F_ROUND, [ROUND0, LATER_DENSE])], ctx=FX11),
    Row("fx-book-all-4-word", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_DENSE=0), SIGNED + [(F_DESC, ["k_round_desc_all<4,false>"]), (F_ROUND, [ROUND0, LATER_WORD])], ctx=FX13),
    Row("fx-book-all-4-dense", "R6", "fx", dict(DVP_MSM_AFF_MIN=32, DVP_MSM_ROUND_DENSE=1), SIGNED + [(F_DESC, ["k_round_desc_all<4,true>"]), (F_ROUND, [ROUND0, LATER_DENSE])], ctx=FX13),
    # the 400 triples: buckets of 3, 6, .. points, a leftover in every bucket of every other round, in dense order
    Row("fx-triples-dense", "T", "fx", dict(DVP_MSM_AFF_MIN=1, DVP_MSM_AFF_BMIN=1, DVP_MSM_ROUND_DENSE=1), SIGNED + [(F_ROUND, [ROUND0, LATER_DENSE])] + reducer(["k_bucket_gather_aff"], []), ctx=FX8),
    Row("fx-proj-mode", "R6", "fx", dict(DVP_MSM_PROJ=1, DVP_MSM_AFF_MIN=32), SIGNED + NO_ROUNDS, ctx=FX11),
    # ---- the reducer on table entries and behind one round, fixed-base (nk = 1 024: the last level fits ACCUM_HEX_MAX and runs on rows of 16;
    # buckets of ~800 points need three levels of fan-in 8, the first two too long for it)
    Row("fx-ra0-fast-lane", "X", "fx", dict(**RA0, **LANE), SIGNED + NO_ROUNDS + reducer(["k_accum_affine_fast<true,false>", "k_accum_affine_rest<true>"], ["k_accum_proj<1>", "k_accum_proj<16>"]), rest=">0", ctx=FX11),
    Row("fx-ra0-fast-quad", "X", "fx", dict(**RA0, **QUAD), SIGNED + NO_ROUNDS + reducer(["k_accum_affine_fast<true,true>", "k_accum_affine_rest<true>"], ["k_accum_proj<4>", "k_accum_proj<16>"]), rest=">0", ctx=FX11),
    Row("fx-ra0-general", "X", "fx", dict(DVP_MSM_ACCUM_FAST=0, DVP_MSM_ACCUM_HEX_MAX=0, **RA0, **LANE), SIGNED + NO_ROUNDS + reducer(["k_accum_affine<true,false>"], ["k_accum_proj<1>"]), rest="==0", ctx=FX11),
    Row("fx-round1-fast", "X", "fx", dict(DVP_MSM_BUCKET_PAIRS_MAX=0, **ONE_ROUND, **QUAD), SIGNED + AFTER_ONE + reducer(["k_accum_affine_fast<false,true>", "k_accum_affine_rest<false>"]), rest=">0", ctx=FX11),
    Row("fx-round1-pairs", "X", "fx", dict(DVP_MSM_BUCKET_PAIRS_MAX=100000, **ONE_ROUND), SIGNED + AFTER_ONE + reducer(["k_bucket_pairs", "k_bucket_rest"], []), rest=">0", ctx=FX11),
    Row("fx-pairs-random", "R6", "fx", dict(DVP_MSM_AFF_MIN=4096, DVP_MSM_BUCKET_PAIRS_MAX=12), SIGNED + reducer(["k_bucket_pairs", "k_bucket_rest"], []), rest="==0", ctx=FX11),
    # sixteen points under the scalars 1 .. 16, signed binary windows of 11 bits: one point per bucket of the lowest window
    Row("fx-singletons", "D", "fx", {}, SIGNED + NO_ROUNDS + reducer(["k_bucket_gather_items"], []), ctx=FX11),
    # ---- merge tree and tail, fixed-base: the signed flavour's tail takes rows of 16 unless DVP_MSM_HEX_MAX = 0
    Row("fx-merge-rows", "R6", "fx", dict(DVP_MSM_HEX_MAX=BIG), SIGNED + [(F_MERGE, ["k_merge<16,true>", "k_merge<16,false>"]), (F_TAIL, ["k_tail<true>"])], ctx=FX11),
    Row("fx-merge-quads", "R6", "fx", dict(DVP_MSM_HEX_MAX=0, DVP_MSM_QUAD_MAX=BIG), SIGNED + [(F_MERGE, ["k_merge<4,true>", "k_merge<4,false>"]), (F_TAIL, ["k_tail<false>"])], ctx=FX11),
]


@pytest.fixture(scope="module")
def inputs(dvp):
    xb, xs, _, _, xexp = mc.exceptional_pairs_input()
    return {"X": (xb, xs, xexp), "R3": mc.random_input(dvp, 3000, 4101), "R6": mc.random_input(dvp, 6000, 9101), "T": mc.triples_input(dvp),
            "D": mc.distinct_input(dvp), "ONE": mc.distinct_input(dvp, 1)}


def run_msm_row(dvp, inputs, row, census=True):
    bases, s, exp = inputs[row.inp]
    fb = None
    if census and row.table:
        dvp.lib.dvp_profile_reset()
    if row.route == "fx":
        with dvp.tune(**row.ctx):
            fb = dvp.curve.FixedBaseMsm(bases)
    try:
        if census and not row.table:
            dvp.lib.dvp_profile_reset()
        with dvp.tune(**row.knobs):
            got = np_to_pt(*fb.run(s)) if fb is not None else np_to_pt(*dvp.curve.multi_scalar_mul(s, bases))
        assert got == exp, row.id
        n_rest = mc.rest_len(dvp)
        if row.rest == ">0":
            assert n_rest > 0, (row.id, n_rest)
        elif row.rest == "==0":
            assert n_rest == 0, (row.id, n_rest)
        if census:
            mc.assert_census(dvp, row.ran, row.idle, row.id)
    finally:
        if fb is not None:
            fb.close()


@pytest.mark.parametrize("row", MSM_ROWS, ids=[r.id for r in MSM_ROWS])
def test_msm_paths(dvp, inputs, row):
    run_msm_row(dvp, inputs, row)


def run_points_sum(dvp, census=True):
    """dvp_points_sum_dev: k_sum_points, the one MSM kernel outside msm_core a single-device entry reaches"""
    import torch

    ks = [5, 7, 11]
    rec = np.zeros((3, 10), dtype=np.uint64)
    for i, k in enumerate(ks):
        rec[i, :8] = to_limbs(list(co.k233_mulgen(k))).reshape(8)
    d = torch.from_numpy(rec.view(np.int64)).cuda()
    out = torch.zeros(10, dtype=torch.int64, device="cuda")
    if census:
        dvp.lib.dvp_profile_reset()
    dvp.check(dvp.lib.dvp_points_sum_dev(d.data_ptr(), 3, out.data_ptr(), out.data_ptr() + 64, torch.cuda.current_stream().cuda_stream))
    h = out.cpu().numpy().view(np.uint64)
    assert not int(h[8]) & 0xFFFFFFFF and tuple(from_limbs(h[:8].reshape(2, 4))) == co.k233_mulgen(sum(ks))
    if census:
        mc.assert_census(dvp, [M + "k_sum_points"], [M + "k_tail<true>", M + "k_tail<false>"])


def test_points_sum_path(dvp):
    run_points_sum(dvp)


# ---- ECFFT -------------------------------------------------------------------------------------------------------------------
E = ec.E
F_BUTTERFLY, F_TOP, F_FUSED = ec.F_BUTTERFLY, ec.F_TOP, ec.F_FUSED
extend_variants, enter_exit_variants = ec.extend_variants, ec.enter_exit_variants


@pytest.fixture(scope="module")
def extend_cases(dvp):
    """log_m -> (device tree, five input vectors, the oracle's five outputs); the reference is computed once"""
    made = {}

    def get(log_m):
        if log_m not in made:
            m = 1 << log_m
            ev = rand_fr_np(5 * m, 31 * log_m).reshape(5, m, 4)
            ev[0, :4] = to_limbs([0, o.P - 1, 1, o.P - 2])
            ot = co.FFTree(log_m + 1)
            want = np.stack([ot.extend(ev[b]) for b in range(5)])
            ot.close()
            made[log_m] = (dvp.ec_fft.FFTree(2 * m), ev, want)
        return made[log_m]

    yield get
    for t, _, _ in made.values():
        t.close()


def run_extend(dvp, nat, extend_cases, log_m, radix, census=True):
    t, ev, want = extend_cases(log_m)
    for batch in (1, 2, 3, 4, 5):
        if census:
            dvp.lib.dvp_profile_reset()
        with nat.tune(DVP_ECFFT_RADIX4=radix):
            out = t.extend(ev[:batch])
        assert np.array_equal(out, want[:batch]), (log_m, radix, batch)
        if census:
            ran, idle = extend_variants(log_m, radix, batch)
            mc.assert_census(dvp, ran, idle, (log_m, radix, batch))


@pytest.mark.parametrize("radix", [3, 2, 1, 0])
@pytest.mark.parametrize("log_m", [12, 13, 14, 15, 16, 17])
def test_extend_paths(dvp, nat, extend_cases, log_m, radix):
    """top layers 1 .. 6: the groupings [1], [2], [3], [3,1], [3,2], [3,3] of the unfused passes, k_extend_top from four layers up
    under DVP_ECFFT_RADIX4 = 3 only, every BATCH instantiation with 1 .. 5 vectors"""
    run_extend(dvp, nat, extend_cases, log_m, radix)


def test_extend_variants_cover_every_butterfly():
    want = set(F_BUTTERFLY) | {E + "k_extend_top<true,0>", E + "k_extend_top<false,0>", E + "k_extend_fused<0>"}
    got = set()
    for log_m in (12, 13, 14, 15, 16, 17):
        for radix in (3, 2, 1, 0):
            for batch in (1, 2, 3, 4, 5):
                got |= set(extend_variants(log_m, radix, batch)[0])
    assert got == want


@pytest.fixture(scope="module")
def enter_exit_cases(dvp):
    made = {}

    def get(log_n):
        if log_n not in made:
            n = 1 << log_n
            c, ev = rand_fr_np(n, 600 + log_n), rand_fr_np(n, 700 + log_n)
            ot = co.FFTree(log_n)
            made[log_n] = (dvp.ec_fft.FFTree(n), c, ev, ot.enter(c), ot.exit(ev))
            ot.close()
        return made[log_n]

    yield get
    for t, *_ in made.values():
        t.close()


def run_enter_exit(dvp, nat, enter_exit_cases, log_n, fold, census=True):
    t, c, ev, want_e, want_x = enter_exit_cases(log_n)
    enter_paths, exit_paths = enter_exit_variants(log_n, fold)
    with nat.tune(DVP_ECFFT_FOLD=fold):
        if census:  # the first call of a flavour builds its tables (with enters and extends of its own): count the second
            t.enter(c), t.exit(ev)
            dvp.lib.dvp_profile_reset()
        e = t.enter(c)
        assert np.array_equal(e, want_e), (log_n, fold)
        if census:
            assert_paths(dvp, enter_paths, ("enter", log_n, fold))
            dvp.lib.dvp_profile_reset()
        x = t.exit(ev)
        assert np.array_equal(x, want_x), (log_n, fold)
        if census:
            assert_paths(dvp, exit_paths, ("exit", log_n, fold))


def assert_paths(dvp, paths, where):
    ran, idle, counts = paths
    mc.assert_census(dvp, ran, idle, where)
    for nm, cnt in counts.items():
        assert mc.launches(dvp, nm) == cnt, (nm, where, mc.launches(dvp, nm), cnt)


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("log_n", [3, 11, 12, 13])
def test_enter_exit_paths(dvp, nat, enter_exit_cases, log_n, fold):
    run_enter_exit(dvp, nat, enter_exit_cases, log_n, fold)


def run_tree_build(dvp, nat, census=True):
    """a fresh tree: its layers (k_leaves, k_next_layer; read back through k_from_mont), the twiddles and twists of its first extend
    (k_build_twiddles, k_twist_layer, k_twist_finish), the tables of its first folded exit and enter, and the 2x2 matrices of the
    tree-file export (k_build_mats, k_mats_export), each against the oracle"""
    log_n = 6
    n = 1 << log_n
    ot = co.FFTree(log_n)
    if census:
        dvp.lib.dvp_profile_reset()
    t = dvp.ec_fft.FFTree(n)
    assert np.array_equal(t.leaves(), ot.leaves())
    if census:
        mc.assert_census(dvp, fam(E, "k_leaves", "k_next_layer", "k_from_mont"), F_FUSED)
        dvp.lib.dvp_profile_reset()
    ev = rand_fr_np(n // 2, 61)
    assert np.array_equal(t.extend(ev), ot.extend(ev))
    if census:
        mc.assert_census(dvp, fam(E, "k_build_twiddles", "k_twist_layer", "k_twist_finish", "k_check_canonical", "k_extend_fused<0>"), F_TOP)
        dvp.lib.dvp_profile_reset()
    c = rand_fr_np(n, 62)
    with nat.tune(DVP_ECFFT_FOLD=1):
        assert np.array_equal(t.exit(c), ot.exit(c))
        assert np.array_equal(t.enter(c), ot.enter(c))
    if census:
        mc.assert_census(dvp, fam(E, "k_exit_tables", "k_c_base", "k_neg_from_mont_even", "k_mul_canon", "k_rho", "k_to_mont", "k_exit_fuse_tables", "k_enter_fuse_tables",
                                  "k_pow_table", "k_exit_leaf", "k_leaf_matmul8"), fam(E, "k_exit_pre", "k_exit_post"))
        dvp.lib.dvp_profile_reset()
    half = n // 2
    for te in (0, 1):
        for w in (0, 1):
            a = np.zeros(((half - 1) * 4, 4), dtype=np.uint64)
            dvp.check(dvp.lib.dvp_debug_ecfft_matrices(t._h, te, w, nat.ptr(a)))
            assert np.array_equal(a.reshape(half - 1, 4, 4), ot.matrices(bool(te), w).reshape(half - 1, 4, 4)), (te, w)
    if census:
        mc.assert_census(dvp, fam(E, "k_build_mats", "k_mats_export"), F_FUSED)
    ot.close()
    t.close()


def test_tree_build_paths(dvp, nat):
    run_tree_build(dvp, nat)


# ---- fr_ops.hip --------------------------------------------------------------------------------------------------------------
R = "fr_ops.hip:"
BI_SHAPES = {0: (512, 16), 1: (256, 8), 2: (256, 4), 3: (512, 8), 4: (128, 8), 5: (128, 4), 6: (256, 16), 7: (1024, 8)}  # DVP_FR_BI_SHAPE
F_BI = [f"{R}k_batch_inverse<{tpb},{ch}>" for tpb, ch in BI_SHAPES.values()]


@pytest.fixture(scope="module")
def bi_case():
    rnd = random.Random(9)
    vals = [rnd.randrange(o.P) for _ in range(20011)]
    for z in (0, 63, 64, 4095, 4096, 8191, 8192, 20010):  # zeros at block edges
        vals[z] = 0
    return vals, o.fr_batch_inverse(vals)


def run_batch_inverse(dvp, nat, bi_case, shape, census=True):
    vals, exp = bi_case
    if census:
        dvp.lib.dvp_profile_reset()
    with nat.tune(DVP_FR_BI_SHAPE=shape):
        b = to_limbs(vals)
        dvp.check(dvp.lib.dvp_fr_batch_inverse(nat.ptr(b), len(vals)))
    assert from_limbs(b) == exp, shape
    if census:
        mine = f"{R}k_batch_inverse<{BI_SHAPES[shape][0]},{BI_SHAPES[shape][1]}>"
        mc.assert_census(dvp, [mine], [x for x in F_BI if x != mine], shape)


@pytest.mark.parametrize("shape", sorted(BI_SHAPES))
def test_batch_inverse_shapes(dvp, nat, bi_case, shape):
    run_batch_inverse(dvp, nat, bi_case, shape)


def run_fr_vectors(dvp, nat, census=True):
    """the Fr vector entries, each against Python integers and each shown to be the kernel that ran"""
    P = o.P
    rnd = random.Random(5)
    n = 257
    a, b = [rnd.randrange(P) for _ in range(n)], [rnd.randrange(P) for _ in range(n)]
    s = rnd.randrange(P)
    va, vb = dvp.fr.vec(a), dvp.fr.vec(b)
    vec = fam(R, "k_vec_mul", "k_vec_scale", "k_vec_axpy", "k_vec_scalar_sub", "k_vec_dot_partial", "k_sum_final", "k_spmv", "k_bary_partial", "k_bary_final")

    def step(fn, exp, ran):
        if census:
            dvp.lib.dvp_profile_reset()
        assert fn() == exp
        if census:
            mc.assert_census(dvp, fam(R, *ran), [x for x in vec if x not in fam(R, *ran)], ran)

    step(lambda: dvp.fr.to_ints(dvp.fr.mul(va, vb)), [x * y % P for x, y in zip(a, b)], ["k_vec_mul"])
    step(lambda: dvp.fr.to_ints(dvp.fr.scale(va, s)), [s * x % P for x in a], ["k_vec_scale"])
    step(lambda: dvp.fr.to_ints(dvp.fr.axpy(va, s, vb)), [(x + s * y) % P for x, y in zip(a, b)], ["k_vec_axpy"])
    step(lambda: dvp.fr.to_ints(dvp.fr.scalar_sub(s, va)), [(s - x) % P for x in a], ["k_vec_scalar_sub"])
    step(lambda: dvp.fr.dot(va, vb), sum(x * y for x, y in zip(a, b)) % P, ["k_vec_dot_partial", "k_sum_final"])
    rows = [[(rnd.randrange(n), rnd.randrange(17)) for _ in range(rnd.randrange(6))] for _ in range(300)]
    coeffs = [rnd.randrange(P) for _ in range(17)]
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint32)
    col = np.array([c for r in rows for c, _ in r], dtype=np.uint32)
    cid = np.array([k for r in rows for _, k in r], dtype=np.uint32)
    step(lambda: dvp.fr.to_ints(dvp.fr.spmv(row_ptr, col, cid, dvp.fr.vec(coeffs), va)), [sum(coeffs[k] * a[c] for c, k in r) % P for r in rows], ["k_spmv"])
    tb = o.domain_tables(o.FFTree(6))
    ev = [rnd.randrange(P) for _ in range(tb["m"])]
    alpha = rnd.randrange(P)
    z_alpha = o.poly_eval(tb["z_poly"], alpha)

    def bary():
        out = np.zeros(4, dtype=np.uint64)
        dvp.check(dvp.lib.dvp_barycentric_eval(nat.ptr(to_limbs(tb["D"])), nat.ptr(to_limbs(tb["bar_wts"])), nat.ptr(to_limbs([z_alpha])),
                                               nat.ptr(to_limbs(ev)), tb["m"], nat.ptr(to_limbs([alpha])), nat.ptr(out)))
        return from_limbs(out[None])[0]

    step(bary, o.lagrange_eval(tb["D"], ev, alpha), ["k_bary_partial", "k_bary_final"])


def test_fr_vector_paths(dvp, nat):
    run_fr_vectors(dvp, nat)


# ---- closure -----------------------------------------------------------------------------------------------------------------
# Diagnostics only.  A production variant no row reaches is a finding, not an entry here.
EXEMPT = {
    M + "k_affine_round<true,true,false>": "TRACE = true: the wave trace of tools/wave_trace.py (dvp_debug_wave_trace)",
    M + "k_affine_round<false,true,false>": "TRACE = true, later rounds, one-word descriptors",
    M + "k_affine_round<false,true,true>": "TRACE = true, later rounds, dense order",
    M + "k_ubench_mul": "microbenchmark (dvp_ubench_gf_mul)",
    M + "k_ubench_gather": "microbenchmark (dvp_ubench_gather)",
    R + "k_ubench_fr30": "microbenchmark (dvp_ubench_fr_mul)",
    # k_sum_points IS reached (dvp_points_sum_dev, above); k_join_points is not: it adds the table part and the one-shot part of a
    # prover's MSM whose fixed-base table a budget cut short, and only dvp_prove reaches it (tests/test_gpu_table_budget.py)
    M + "k_join_points": "only inside a prover under a table budget: no MSM / ECFFT / Fr entry of a single device launches it",
}
# k_build_sqr_tables fills a device's squaring tables at the process's first MSM and never again: a launch of it can only be witnessed in
# a fresh process
ONCE_PER_PROCESS = M + "k_build_sqr_tables"
CHILD = r"""
import importlib, os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
dvp = importlib.import_module("dv-pari_amd")
import c_oracle as co, msm_cases as mc
from util import np_to_pt
dvp.lib.dvp_profile_reset()
bases, s, exp = mc.distinct_input(dvp)
assert np_to_pt(*dvp.curve.multi_scalar_mul(s, bases)) == exp
print("launches", mc.launches(dvp, sys.argv[2]))
"""


def test_every_variant_runs(dvp, nat, inputs, extend_cases, enter_exit_cases, bi_case):
    dvp.lib.dvp_profile_reset()
    for row in MSM_ROWS:
        run_msm_row(dvp, inputs, row, census=False)
    run_points_sum(dvp, census=False)
    for log_m in (12, 13, 14, 15, 16, 17):
        for radix in (3, 2, 1, 0):
            run_extend(dvp, nat, extend_cases, log_m, radix, census=False)
    for log_n in (3, 11, 12, 13):
        for fold in (1, 0):
            run_enter_exit(dvp, nat, enter_exit_cases, log_n, fold, census=False)
    run_tree_build(dvp, nat, census=False)
    for shape in sorted(BI_SHAPES):
        run_batch_inverse(dvp, nat, bi_case, shape, census=False)
    run_fr_vectors(dvp, nat, census=False)
    got = mc.census(dvp)
    assert len(got) > 130 and set(EXEMPT) <= set(got) and ONCE_PER_PROCESS in got
    never = sorted(nm for nm, n in got.items() if n == 0 and nm not in EXEMPT and nm != ONCE_PER_PROCESS)
    assert not never, never
    assert all(got[nm] == 0 for nm in EXEMPT), {nm: got[nm] for nm in EXEMPT if got[nm]}  # an entry that runs has no business on the list
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = subprocess.run([sys.executable, "-c", CHILD, root, ONCE_PER_PROCESS], capture_output=True, text=True, timeout=300)
    assert child.returncode == 0 and "launches 1" in child.stdout, (child.returncode, child.stdout[-400:], child.stderr[-400:])
