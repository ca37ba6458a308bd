"""The DEVICE build of every Fr function of csrc/fr.cuh (dvp_debug_fr_op, on_device = 1: one element per lane, 256-thread workgroups,
the explicit v_mad_u64_u32 chains of the kernels included) against exact Python integers on the chosen operands of fr_cases.py,
and byte for byte against the host build of the same function.  Integer equality only."""
import pytest

import fr_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op", fc.OPS)
def test_device_op_vs_integers_and_host(dvp, op):
    got = fc.run_op(dvp, op, True)
    fc.assert_same(op, got, fc.expected(op))
    fc.assert_same(op, got, fc.run_op(dvp, op, False), "host build")


def test_zero_inverts_to_zero_on_device(dvp):
    for op in ("inv", "inv_gcd_raw", "inv_fermat"):
        assert dvp.fr.debug_op(op, [fc.pack([0, 1, 0])], True)[0][:32] == bytes(32)


def test_single_element_and_exact_workgroups(dvp):
    """lengths 1, 256 and 257 next to the ragged ones above"""
    a, b = fc.inputs("mul")
    want = fc.expected("mul")[0]
    for n in (1, 256, 257):
        assert dvp.fr.debug_op("mul", [a[:32 * n], b[:32 * n]], True)[0] == want[:32 * n], n
