"""CPU tests of the table budget: the planner behind dvp_prover_set_table_budget (dvp_table_plan, a pure host function), the
status text of DVP_ENOMEM and the python binding.  No GPU call is made here.

The planner's contract (include/dvpari.h, dvp_prover_set_table_budget): MSM 1 (4m terms) is served first, then MSM 0; at most one
of the two is partly covered, by a table over a prefix; a prefix shorter than DVP_MSM_FIXED_MIN gets no table; the bytes of the
tables -- rows x covered x 64, rows as the fixed-base context settles them for that count -- never exceed the budget."""
import random

import pytest

LOGS = list(range(13, 25))
FIXED_MINS = [1, 1 << 12, 1 << 16]  # 2^16 is the default


def sizes(log_m):
    """(terms of MSM 0, terms of MSM 1) of bench.py's dense circuit shape: n_wires = m"""
    m = 1 << log_m
    return 2 * m, 4 * m


def budgets(full, rnd):
    """0 .. above the full size: the end points, the neighbourhood of every eighth and random points"""
    out = {0, 1, 63, 64, 65, full - 1, full, full + 1, 2 * full, (1 << 64) - 1}
    for k in range(1, 8):
        b = full * k // 8
        out |= {b - 1, b, b + 1}
    out |= {rnd.randrange(full + 1) for _ in range(40)}
    return sorted(b for b in out if b >= 0)


def tableable(n, fixed_min):
    return n if n >= fixed_min else 0


@pytest.mark.parametrize("fixed_min", FIXED_MINS)
def test_planner_properties(dvp, fixed_min):
    rnd = random.Random(fixed_min)
    with dvp.tune(DVP_MSM_FIXED_MIN=fixed_min):
        for log_m in LOGS:
            s0, s1 = sizes(log_m)
            (f0, f1), (fb0, fb1) = dvp.table_plan(s0, s1, None)
            # no limit: everything DVP_MSM_FIXED_MIN lets into a table is covered
            assert (f0, f1) == (tableable(s0, fixed_min), tableable(s1, fixed_min)), log_m
            full = fb0 + fb1
            assert fb0 % 64 == 0 and fb1 % 64 == 0
            if f1:
                assert 8 <= fb1 // (64 * f1) <= 31  # a row count the recode can address
            prev = (0, 0)
            for b in budgets(max(full, 1 << 20), rnd):
                (c0, c1), (b0, b1) = dvp.table_plan(s0, s1, b)
                where = (log_m, fixed_min, b)
                assert b0 + b1 <= b, where                                   # never more bytes than the budget
                assert c0 <= s0 and c1 <= s1, where
                assert (c0 == 0) == (b0 == 0) and (c1 == 0) == (b1 == 0), where
                assert c0 == 0 or c0 >= fixed_min, where                     # no table below DVP_MSM_FIXED_MIN
                assert c1 == 0 or c1 >= fixed_min, where
                assert not (0 < c0 < s0 and 0 < c1 < s1), where              # at most one MSM partly covered
                assert c0 == 0 or c1 == f1, where                            # MSM 1 first
                assert c1 >= prev[1] and c0 >= prev[0], where                # monotone in the budget
                if b >= full:
                    assert (c0, c1) == (f0, f1) and (b0, b1) == (fb0, fb1), where
                prev = (c0, c1)


def test_planner_bytes_are_rows_times_count(dvp):
    """bytes = rows x covered x 64 with a whole row count, and a budget one byte short of a plan's bytes gives a smaller plan"""
    with dvp.tune(DVP_MSM_FIXED_MIN=1):
        s0, s1 = sizes(20)
        (_, _), (fb0, fb1) = dvp.table_plan(s0, s1, None)
        for b in (fb1 // 3, fb1, fb1 + fb0 // 2, fb1 + fb0):
            (c0, c1), (b0, b1) = dvp.table_plan(s0, s1, b)
            for c, nb in ((c0, b0), (c1, b1)):
                assert c == 0 or nb % (64 * c) == 0
            (d0, d1), (e0, e1) = dvp.table_plan(s0, s1, b0 + b1 - 1)
            assert e0 + e1 < b0 + b1 and (d0, d1) < (c0, c1) or b0 + b1 == 0
        # the 2^20 figure of the README: 12 rows, 768 B per base
        assert fb1 == 12 * s1 * 64 and fb0 == 12 * s0 * 64
        # forced window bits change the row count the planner uses
        with dvp.tune(DVP_MSM_FIXED_C=10):
            (_, c1), (_, b1) = dvp.table_plan(s0, s1, None)
            assert c1 == s1 and b1 == 24 * s1 * 64  # ceil(234 / 10) = 24 rows


def test_planner_zero_sizes_and_null(dvp):
    assert dvp.table_plan(0, 0, None) == ((0, 0), (0, 0))
    assert dvp.lib.dvp_table_plan(16, 16, 0, None, None) == -1


def test_enomem_has_a_name(dvp):
    assert dvp.lib.dvp_strerror(-7) != dvp.lib.dvp_strerror(-12345)
    assert b"memory" in dvp.lib.dvp_strerror(-7)
    e = dvp.DvpError(-7, "somewhere")
    assert e.status == -7 and e.name == "DVP_ENOMEM" and "DVP_ENOMEM" in str(e)
    assert dvp.DvpError(-4, "x").name == "DVP_EHIP"


def test_new_symbols_are_bound(dvp, nat):
    for name in ("dvp_prover_set_table_budget", "dvp_prover_msm_coverage", "dvp_table_plan"):
        assert name in nat.EXPORTED, name
    for knob in ("DVP_TABLE_BUDGET_BYTES", "DVP_MSM_TABLE_REFUSE"):
        import ctypes as C
        v = C.c_longlong(7)
        assert dvp.lib.dvp_tune_get(knob.encode(), C.byref(v)) == 0
    assert hasattr(dvp.proving.Prover, "set_table_budget") and hasattr(dvp.proving.Prover, "msm_coverage")
