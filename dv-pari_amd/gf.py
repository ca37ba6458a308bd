"""GF(2^233) and K-233 point formulas one function at a time: the test-only entry dvp_debug_gf_op (include/dvpari_internal.h)."""
import ctypes as C

import numpy as np

from ._native import lib, check

# enum dvp_gf_form
FORMS = {"reg": 0, "lds": 1, "ldsq": 2, "ldsh": 3, "ldsk": 4}
LDS_FORMS = ("lds", "ldsq", "ldsh", "ldsk")
LANES = {"reg": 1, "lds": 1, "ldsq": 4, "ldsh": 16, "ldsk": 1}  # lanes per element: out[k] holds n x LANES values
# param & 0xff of "sqr_tab": table -> (selector, squarings; None = the half-trace); | SQR_TAB_WIDE: gf_sqr_tab_wide
SQR_TABS = {"t29": (0, 29), "t58": (1, 58), "t116": (2, 116), "th": (3, None), "t14": (4, 14), "t7": (5, 7)}
SQR_TAB_WIDE = 0x100

# enum dvp_gf_op: name -> (number, inputs, value outputs, has a flag in out[3])
DEBUG_OPS = {name: (k, n_in, n_out, flag) for k, (name, n_in, n_out, flag) in enumerate([
    ("add", 2, 1, False), ("mul", 2, 1, False), ("mul2", 3, 2, False), ("sqr", 1, 1, False), ("sqr_n", 1, 1, False),
    ("reduce16_15", 2, 1, False), ("reduce16_14", 2, 1, False), ("sqr_tab", 1, 1, False), ("sqr_n_fast", 1, 1, False),
    ("inv", 1, 1, False), ("inv_fast", 1, 1, False), ("sqrt", 1, 1, False), ("trace", 1, 1, False), ("halftrace", 1, 1, False),
    ("ld_dbl", 3, 3, False), ("ld_madd", 5, 3, False), ("ld_madd_fast", 5, 3, True), ("ld_add_aff_aff", 4, 3, False),
    ("ld_add", 6, 3, False), ("ld_add_nodbl", 6, 3, True), ("lam_from_ld", 3, 3, False), ("lam_to_ld", 3, 3, False),
    ("lam_dbl", 3, 3, False), ("lam_add", 6, 3, True), ("ld_frob_n", 3, 3, False), ("ld_to_aff", 3, 2, True)])}
# the forms an op exists in
ALL_FORM_OPS = ("mul", "ld_dbl", "ld_madd", "ld_add")
LDS_FORM_OPS = ("mul2", "inv_fast", "ld_madd_fast", "ld_add_aff_aff", "ld_add_nodbl", "lam_from_ld", "lam_to_ld", "lam_dbl", "lam_add")


def op_forms(name: str) -> tuple:
    return ("reg",) + LDS_FORMS if name in ALL_FORM_OPS else LDS_FORMS if name in LDS_FORM_OPS else ("reg",)


def debug_op(name: str, form: str, inputs, param: int = 0):
    """dvp_debug_gf_op: one function of csrc/gf233.cuh / csrc/k233.cuh per element, on the device.  inputs: one bytes object of
    n x 32 bytes (raw little-endian 256-bit values) per operand.  Returns the value outputs, then the flag output if the op has one,
    as bytes of n x LANES[form] x 32 bytes each (value e * LANES + r = lane r's copy of element e)."""
    op, n_in, n_out, flag = DEBUG_OPS[name]
    assert len(inputs) == n_in and len({len(b) for b in inputs}) == 1 and len(inputs[0]) % 32 == 0
    n = len(inputs[0]) // 32
    ins = [np.frombuffer(bytes(b), dtype="<u8") for b in inputs]
    outs = [np.zeros(4 * n * LANES[form], dtype=np.uint64) for _ in range(n_out + (1 if flag else 0))]
    pin = (C.c_void_p * 6)(*[a.ctypes.data for a in ins])
    slots = [a.ctypes.data for a in outs[:n_out]] + [None] * (4 - n_out)
    if flag:
        slots[3] = outs[n_out].ctypes.data
    pout = (C.c_void_p * 4)(*slots)
    check(lib.dvp_debug_gf_op(op, FORMS[form], pin, n, int(param), pout), f"dvp_debug_gf_op({name}, {form})")
    return [a.tobytes() for a in outs]
