"""Which ECFFT kernel variants a size and a knob select, restated from csrc/ecfft_extend.cuh (extend_io) and ecfft_enter_exit.cuh (enter_core, exit_core) for the
launch census: the path tests assert these beside their oracle comparisons."""
E = "ecfft.hip:"
FUSE_LOG, TOP_MAX = 11, 9  # layers one k_extend_fused block / one k_extend_top launch covers


def fam(*names):
    return [E + n for n in names]


F_BUTTERFLY = [f"{E}{k}<{b},{d}>" for k in ("k_butterfly", "k_butterfly4", "k_butterfly8") for b in (1, 2, 3, 4) for d in ("true", "false")]
F_TOP = fam("k_extend_top<true,0>", "k_extend_top<false,0>", "k_extend_top<false,1>", "k_extend_top<false,2>", "k_extend_top<false,3>")
F_FUSED = fam("k_extend_fused<0>", "k_extend_fused<1>", "k_extend_fused<2>", "k_extend_fused<3>")
F_FOLDED = fam("k_extend_fused<1>", "k_extend_fused<2>", "k_extend_fused<3>", "k_extend_top<false,1>", "k_extend_top<false,2>", "k_extend_top<false,3>")


def extend_variants(log_m, radix, batch):
    """(ran, idle) of an extend of `batch` vectors of 2^log_m values: the 11 bottom layers are one k_extend_fused<0>; of the
    top = log_m - 11 layers above them DVP_ECFFT_RADIX4 = 3 takes up to nine in one k_extend_top pair when there are at least four, and
    what is left goes in passes of three (radix >= 2), two (radix >= 1) or one layer, each pass once decomposing and once recombining;
    a batch of 2 .. 4 vectors selects the BATCH instantiation, anything else BATCH = 1"""
    top = max(log_m - FUSE_LOG, 0)
    tl = min(top, TOP_MAX) if radix >= 3 and top >= 4 else 0
    left, ran = top - tl, [E + "k_extend_fused<0>"]
    if tl:
        ran += fam("k_extend_top<true,0>", "k_extend_top<false,0>")
    b = batch if 2 <= batch <= 4 else 1
    while left > 0:
        g = 3 if radix >= 2 and left >= 3 else 2 if radix >= 1 and left >= 2 else 1
        kern = {3: "k_butterfly8", 2: "k_butterfly4", 1: "k_butterfly"}[g]
        ran += [f"{E}{kern}<{b},true>", f"{E}{kern}<{b},false>"]
        left -= g
    return ran, [x for x in F_BUTTERFLY + F_TOP + F_FUSED if x not in ran]


def enter_exit_variants(log_n, fold):
    """((ran, idle, exact counts) of enter, (ran, idle, exact counts) of exit) on a tree of 2^log_n leaves, its tables built.

    Both walk the levels h = n / 2, n / 4, .. 1 (sub-vectors of h values, an extend of h values each).  Folded (DVP_ECFFT_FOLD = 1),
    from eight leaves up the three bottom levels h = 4, 2, 1 are one k_leaf_matmul8, and a level's pointwise stages ride in the last
    launch of its extend (enter: ExtIo<3>) or in the first and last launches of its four extends (exit: ExtIo<1> twice, ExtIo<2>, one
    plain): k_extend_fused while the vector fits one block (h <= 2048), k_extend_top from h = 4096.  ext_io_ok refuses the enter
    combine at h = 2048 (one vector per block, no top launch to pair two vectors in) and everything at h = 1: those levels keep
    k_enter_combine, and a folded exit's h = 1 level is k_exit_leaf.  Unfolded: k_enter_combine per level, k_exit_pre / _mid twice and
    k_exit_mulc / _post once per level, plain extends (ExtIo<0>) only."""
    leaf8 = bool(fold) and log_n >= 3
    hs = [1 << j for j in range(3 if leaf8 else 0, log_n)]  # the levels outside k_leaf_matmul8
    e_ran, e_cnt, x_ran, x_cnt = [], {}, [], {}
    if fold:
        if leaf8:
            e_ran += fam("k_leaf_matmul8")
            x_ran += fam("k_leaf_matmul8")
        folded_e = [h for h in hs if h >= 2 and h != 2048]
        if any(h <= 1024 for h in folded_e):
            e_ran += fam("k_extend_fused<3>")
        if any(h >= 4096 for h in folded_e):
            e_ran += fam("k_extend_top<false,3>", "k_extend_top<true,0>")
        e_cnt[E + "k_enter_combine"] = sum(1 for h in hs if h == 1 or h == 2048)
        folded_x = [h for h in hs if h >= 2]
        if any(h <= 2048 for h in folded_x):
            x_ran += fam("k_extend_fused<1>", "k_extend_fused<2>")
        if any(h >= 4096 for h in folded_x):
            x_ran += fam("k_extend_top<false,1>", "k_extend_top<false,2>", "k_extend_top<true,0>")
        x_cnt[E + "k_exit_leaf"] = sum(1 for h in hs if h == 1)
        for k in ("k_exit_pre", "k_exit_mid", "k_exit_mulc", "k_exit_post"):
            x_cnt[E + k] = 0
    else:
        e_cnt[E + "k_enter_combine"] = log_n
        x_cnt.update({E + "k_exit_pre": 2 * log_n, E + "k_exit_mid": 2 * log_n, E + "k_exit_mulc": log_n, E + "k_exit_post": log_n})
        if log_n >= 2:
            e_ran += fam("k_extend_fused<0>")
            x_ran += fam("k_extend_fused<0>")
    e_idle = [x for x in F_FOLDED + fam("k_leaf_matmul8", "k_exit_leaf", "k_exit_pre", "k_exit_mid", "k_exit_mulc", "k_exit_post") if x not in e_ran]
    x_idle = [x for x in F_FOLDED + fam("k_leaf_matmul8", "k_enter_combine") if x not in x_ran]
    return (e_ran, e_idle, e_cnt), (x_ran, x_idle, x_cnt)
