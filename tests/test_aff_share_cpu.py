"""CPU tests of the pair rounds' choice between one field inversion per workgroup and one per wave (dvp_aff_share_plan, a pure host
function: msm.hip calls the same code for every round it launches)."""
import pytest

CHIP_FULL = 196608 * 8  # resident pair-round threads of an MI355X x DVP_MSM_AFF_BMIN


def plan(dvp, mode, tpb, planned, share_min=0, chip_full=CHIP_FULL):
    return dvp.lib.dvp_aff_share_plan(mode, tpb, planned, share_min, chip_full)


def test_exported(dvp):
    assert hasattr(dvp.lib, "dvp_aff_share_plan")


@pytest.mark.parametrize("tpb", [64, 128, 256])
def test_never_and_always(dvp, tpb):
    for planned in (0, 1, CHIP_FULL - 1, CHIP_FULL, 1 << 40):
        assert plan(dvp, 0, tpb, planned) == 0
        assert plan(dvp, 1, tpb, planned) == (0 if tpb == 64 else 1)  # one wave has nobody to share with


def test_auto_threshold_edges(dvp):
    for tpb in (128, 256):
        assert plan(dvp, 2, tpb, CHIP_FULL - 1) == 0
        assert plan(dvp, 2, tpb, CHIP_FULL) == 1
        assert plan(dvp, 2, tpb, CHIP_FULL + 1) == 1
        # an explicit DVP_MSM_AFF_SHARE_MIN replaces the chip-full
        assert plan(dvp, 2, tpb, 999, share_min=1000) == 0
        assert plan(dvp, 2, tpb, 1000, share_min=1000) == 1
        assert plan(dvp, 2, tpb, CHIP_FULL, share_min=CHIP_FULL + 1) == 0
        assert plan(dvp, 2, tpb, 0, share_min=0, chip_full=0) == 1
    assert plan(dvp, 2, 64, 1 << 40) == 0


def test_unknown_modes_and_sizes_stay_private(dvp):
    for mode in (-1, 3, 1 << 40):
        assert plan(dvp, mode, 256, 1 << 40) == 0
    for tpb in (0, 32, 192, 512):
        assert plan(dvp, 1, tpb, 1 << 40) == 0
