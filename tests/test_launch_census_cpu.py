"""The launch census cannot be bypassed and knows every kernel (no GPU needed): the one textual hipLaunchKernelGGL of csrc/ is the
wrapper's own (common.h: Launch<K>::go, behind DVP_LAUNCH), and dvp_debug_launch_names -- which touches no device -- lists at least
one variant for every __global__ kernel of the sources, under the file that launches it."""
import ctypes as C
import os
import re

import pytest

from msm_cases import launch_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dv-pari_amd", "csrc")
LIB = os.path.join(ROOT, "dv-pari_amd", "libdvpari_hip.so")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h", ".cuh")))


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_only_the_wrapper_launches():
    hits = [(f, i + 1) for f in SOURCES for i, line in enumerate(_text(f).splitlines()) if "hipLaunchKernelGGL" in line or "<<<" in line]
    assert len(hits) == 1 and hits[0][0] == "common.h", hits
    body = _text("common.h")
    at = body.index("hipLaunchKernelGGL")
    assert body.rindex("struct Launch<K>", 0, at) > body.rindex("struct LaunchSite", 0, at)  # inside the wrapper's definition
    assert "fetch_add(1, std::memory_order_relaxed)" in body[body.rindex("struct Launch<K>", 0, at):at]  # behind the count


def _kernels(text):
    """names of the __global__ functions a source defines: the identifier in front of the parameter list that follows the attribute
    (comments stripped; __launch_bounds__(...) and __attribute__((...)) stand between the two)"""
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    out = []
    for m in re.finditer(r"__global__", text):
        rest = text[m.end():m.end() + 600]
        rest = re.sub(r"__launch_bounds__\s*\([^()]*(\([^()]*\))?[^()]*\)", " ", rest)
        rest = re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)", " ", rest)
        k = re.match(r"\s*(?:static\s+)?void\s+([A-Za-z_]\w*)\s*\(", rest)
        assert k, rest[:120]
        out.append(k.group(1))
    return out


def _includers():
    """header -> the .hip / .cpp sources whose translation unit holds it, through their #include "..." lines and those of the headers"""
    direct = {f: set(re.findall(r'^#include "(\w+\.(?:cuh|h))"', _text(f), flags=re.M)) for f in SOURCES}
    out = {}
    for f in SOURCES:
        if not f.endswith((".hip", ".cpp")):
            continue
        seen, todo = set(), [f]
        while todo:
            for h in direct.get(todo.pop(), ()):
                if h not in seen:
                    seen.add(h)
                    todo.append(h)
        for h in seen:
            out.setdefault(h, set()).add(f)
    return out


@pytest.fixture(scope="module")
def names():
    if not os.path.exists(LIB):
        pytest.skip("libdvpari_hip.so is not built")
    return launch_names(C.CDLL(LIB))


def test_every_kernel_has_a_census_name(names):
    assert len(names) == len(set(names)) and all(re.fullmatch(r"[\w.]+\.hip:k\w*(<.*>)?", nm) for nm in names), names
    listed = {}
    for nm in names:
        f, v = nm.split(":", 1)
        listed.setdefault(f, set()).add(v.split("<", 1)[0])
    inc = _includers()
    found = 0
    for f in SOURCES:
        for k in _kernels(_text(f)):
            found += 1
            # a kernel defined in a header is launched from the files that include it: the one source where there is only one (the stage
            # headers of msm.hip), any listed file where several sources share the header
            by = sorted(inc.get(f, ()))
            where = [f] if f.endswith(".hip") else by if len(by) == 1 else sorted(listed)
            assert any(k in listed.get(w, ()) for w in where), (f, k, where)
    stages = sorted(f for f in SOURCES if re.fullmatch(r"msm_\w+\.cuh", f))
    assert len(stages) >= 8 and all(inc.get(h) == {"msm.hip"} for h in stages), {h: inc.get(h) for h in stages}
    # the same for prove.hip's phase headers; its kernels live in prove_kernels.cuh and are listed under prove.hip
    phases = sorted(f for f in SOURCES if re.fullmatch(r"prove_\w+\.cuh", f))
    assert len(phases) >= 7 and all(inc.get(h) == {"prove.hip"} for h in phases), {h: inc.get(h) for h in phases}
    prove_kernels = _kernels(_text("prove_kernels.cuh"))
    assert len(prove_kernels) >= 16 and set(prove_kernels) <= listed["prove.hip"], set(prove_kernels) - listed["prove.hip"]
    assert not _kernels(_text("prove.hip")) and "k_bary3_partial" not in listed["prove.hip"]
    # and for ecfft.hip's stage headers: every kernel of theirs is listed under ecfft.hip, which defines none itself
    ecfft = sorted(f for f in SOURCES if re.fullmatch(r"ecfft_\w+\.cuh", f))
    assert len(ecfft) >= 6 and all(inc.get(h) == {"ecfft.hip"} for h in ecfft), {h: inc.get(h) for h in ecfft}
    ecfft_kernels = [k for h in ecfft for k in _kernels(_text(h))]
    assert len(ecfft_kernels) >= 30 and set(ecfft_kernels) <= listed["ecfft.hip"], set(ecfft_kernels) - listed["ecfft.hip"]
    assert not _kernels(_text("ecfft.hip"))
    # the scan itself sees the kernels: msm.hip's are its own and those of the headers only it includes
    assert found > 100 and sum(len(_kernels(_text(f))) for f in ["msm.hip"] + sorted(h for h, by in inc.items() if by == {"msm.hip"})) > 40


def test_names_carry_instantiated_arguments(names):
    """launches inside templated host code and macros name the arguments they were instantiated with, never a parameter's spelling"""
    for nm in names:
        if "<" in nm:
            args = nm[nm.index("<") + 1:-1].split(",")
            assert all(re.fullmatch(r"true|false|-?\d+u?l*|\(\w+(::\w+)*\)\d+|unsigned (int|short)", a) for a in args), nm
    for want in ("msm.hip:k_merge<16,true>", "msm.hip:k_merge<1,false>", "msm.hip:k_accum_affine_fast<true,false>", "msm.hip:k_affine_round<false,false,true>",
                 "msm.hip:k_round_desc_all<64,true>", "ecfft.hip:k_butterfly8<4,true>", "ecfft.hip:k_extend_top<false,3>", "fr_ops.hip:k_batch_inverse<256,16>"):
        assert want in names, want


def test_unknown_census_name_is_einval(names):
    lib = C.CDLL(LIB)
    lib.dvp_profile_read.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    ms, n = C.c_double(0), C.c_uint64(7)
    assert lib.dvp_profile_read(b"launch:msm.hip:k_no_such_kernel", C.byref(ms), C.byref(n)) == -1
    assert lib.dvp_profile_read(b"launch:msm.hip:k_merge<16,true>", C.byref(ms), C.byref(n)) == 0 and n.value == 0 and ms.value == 0
    short = C.create_string_buffer(8)  # a short buffer is filled as far as it goes and the full length is still returned
    need = lib.dvp_debug_launch_names(short, 8)
    assert need == len("\n".join(names)) + 2 and len(short.value) == 7
