"""What the winner search's three launchers selected before plan_wta / plan_wta_right / plan_wta_rel (mgm_amd/csrc/mgm_planner.h)
replaced their logic: a restatement of launch_wta, of the pruning test of run_wta, of launch_wta_right and of launch_wta_rel as
they stood in the commit before the planner -- the cascade in its order, the three grid caps where they were.
tests/test_wta_plan.py holds the planner against it field by field.

A request is a tuple in the order of the C++ struct's fields (WTA_FIELDS, RIGHT_FIELDS, REL_FIELDS); a choice is a tuple in
the order of the harness's output (WTA_OUT, RIGHT_OUT, REL_OUT)."""

WTA_FIELDS = ("npix L Lreal NDIR lpl cbytes compact refine want_S window ragged in_last_run last_min lr_is_last pix0_zero padded nvol_mod32 "
              "num_cu sw_prune sw_prune_ppw sw_prune_wg sw_wg_per_cu sw_packed sw_wide4 sw_quad").split()
WTA_OUT = "family LPL PPW EXACT MAXD SUB ALLD grid prune".split()
RIGHT_FIELDS = "L Lk nx ny vnx dmin dmax num_cu sw_right_seg sw_right_any".split()
RIGHT_OUT = "family LPL PPW seg ring grid".split()
REL_FIELDS = "npix num_cu slots cb".split()
REL_OUT = "SPL CB grid".split()

REFUSE, PLAIN, PACKED, QUAD, ANY, PRUNED = range(6)   # WtaFamily
RIGHT_REFUSE, RIGHT_STREAM, RIGHT_DIAGONAL = range(3)  # WtaRightFamily
MAX_DIRS = 8


def pass_lpl(L):
    """mgm_pass.hip: disparities per lane the kernels are instantiated for."""
    lpl = (L + 63) // 64
    if lpl == 5:
        return 6
    if lpl == 7:
        return 8
    if lpl <= 8:
        return lpl
    return 12 if lpl <= 12 else (16 if lpl <= 16 else (24 if lpl <= 24 else 32))


def wta(q):
    (npix, L, Lreal, NDIR, lpl, cbytes, compact, refine, want_S, window, ragged, in_last_run, last_min, lr_is_last, pix0_zero, padded,
     nvol_mod32, num_cu, sw_prune, prune_ppw, prune_wg, wg_per_cu, sw_packed, sw_wide4, sw_quad) = q
    cus = num_cu if num_cu > 0 else 256
    # run_wta: WtaParams::Lmin is passed iff ... (the launch of a disabled search wrote no minima: `last_min` came out of
    # plan_wta_prune, which was asked with the same switch in the same call)
    lmin = bool(sw_prune and in_last_run and last_min and not want_S and not window and not ragged and refine <= 1 and not padded and pix0_zero
                and compact and cbytes == 1 and L == 256 and lr_is_last)
    if lmin:  # launch_wta, `if (p.Lmin)`
        if L != 256 or Lreal != 256 or not compact or cbytes != 1 or want_S or window or ragged or refine > 1 or nvol_mod32 != 0:
            return (REFUSE, 0, 0, 0, 0, 0, 0, 0, 1)
        pw = 1 if (prune_ppw == 1 or NDIR not in (4, 8)) else 2
        nb = min((npix + 4 * pw - 1) // (4 * pw), cus * (prune_wg if prune_wg > 0 else 64))
        if NDIR == 8:
            inst = (pw, 8, 1)
        elif NDIR == 4:
            inst = (pw, 4, 1)
        elif NDIR < 4:
            inst = (1, 4, 0)
        else:
            inst = (1, 8, 0)
        return (PRUNED, 0, inst[0], 0, inst[1], 0, inst[2], nb, 1)
    nb = (npix + 3) // 4
    per_cu = max(wg_per_cu, 0)
    use_packed = bool(sw_packed and Lreal == L and L in (128, 64) and npix % (256 // L) == 0)
    nb = min(nb, cus * (per_cu if per_cu else (128 if use_packed else 768)))
    if L > 32 * 64:
        return (ANY, 0, 0, 0, 0, 0, 0, nb, 0)
    if sw_quad and Lreal == L and L in (192, 384) and npix % (768 // L) == 0 and not window and not ragged and refine <= 1:
        nq = min((npix // (768 // L) + 3) // 4, cus * (per_cu if per_cu else 256))
        return (QUAD, L // 64, 0, 0, 4 if NDIR <= 4 else MAX_DIRS, 0, 0, nq, 0)
    if use_packed:
        return (PACKED, 4, 4 if NDIR <= 4 else 2, 1, 4 if NDIR <= 4 else MAX_DIRS, 2 if L == 128 else 4, 0, nb, 0)
    case = {1: 4, 2: 4, 3: 2, 4: 3, 6: 1, 8: 1}  # WTA_CASE(LPL, PPW)
    if lpl in case:
        if L == 64 * lpl and NDIR <= 4 and sw_wide4:
            return (PLAIN, lpl, 2 * case[lpl], 1, 4, 1, 0, nb, 0)
        if L == 64 * lpl:
            return (PLAIN, lpl, case[lpl], 1, MAX_DIRS, 1, 0, nb, 0)
        return (PLAIN, lpl, 1, 0, MAX_DIRS, 1, 0, nb, 0)
    if lpl in (12, 16):
        return (PLAIN, lpl, 1, 1 if L == 64 * lpl else 0, MAX_DIRS, 1, 0, nb, 0)
    if lpl in (24, 32):
        return (PLAIN, lpl, 1, 0, MAX_DIRS, 1, 0, nb, 0)
    return (REFUSE, 0, 0, 0, 0, 0, 0, nb, 0)


def wta_right(q):
    L, Lk, nx, ny, vnx, dmin, dmax, num_cu, seg_tune, force_any = q
    if L < 1 or Lk < L or nx < 1 or ny < 1 or vnx < 1 or dmax - dmin + 1 != L:
        return (RIGHT_REFUSE, 0, 0, 0, 0, 0)
    cus = num_cu if num_cu > 0 else 256
    lpl = Lk // 64 if Lk % 64 == 0 else 0
    if force_any or lpl not in (1, 2, 3, 4, 6, 8, 12, 16):
        return (RIGHT_DIAGONAL, 0, 0, 0, 0, min((vnx * ny + 3) // 4, cus * 64))
    want = (4 * cus + ny - 1) // ny
    seg = max((vnx + want - 1) // want, max(64, L))
    if seg_tune > 0:
        seg = seg_tune
    seg = min(seg, vnx)
    nb = ny * ((vnx + seg - 1) // seg)
    if nb > 0x7fffffff:
        return (RIGHT_REFUSE, 0, 0, seg, 0, nb)
    ppw = 2 if lpl <= 4 else 1
    ring = 64
    while ring < L - 1 + 2 * 4 * ppw:
        ring *= 2
    return (RIGHT_STREAM, lpl, ppw, seg, ring, nb)


def wta_rel(q):
    npix, num_cu, slots, cb = q
    grid = max(1, min((npix + 15) // 16, num_cu * 64))
    return (8 if slots == 128 else 4, 4 if cb == 4 else (2 if cb == 2 else 1), grid)


def instance(kind, choice):
    """The kernel instance a choice names, as the source spells it (None: a refusal)."""
    b = lambda v: "true" if v else "false"
    if kind == "wta":
        family, LPL, PPW, EXACT, MAXD, SUB, ALLD = choice[:7]
        return {REFUSE: None, ANY: "k_wta_any", QUAD: "k_wta_q<%d,%d>" % (64 * LPL, MAXD), PRUNED: "k_wta_pruned<%d,%d,%s>" % (PPW, MAXD, b(ALLD)),
                PLAIN: "k_wta<%d,%d,%s,%d,%d>" % (LPL, PPW, b(EXACT), MAXD, SUB), PACKED: "k_wta<%d,%d,%s,%d,%d>" % (LPL, PPW, b(EXACT), MAXD, SUB)}[family]
    if kind == "right":
        return {RIGHT_REFUSE: None, RIGHT_DIAGONAL: "k_wta_right_any", RIGHT_STREAM: "k_wta_right<%d,%d>" % (choice[1], choice[2])}[choice[0]]
    return "k_wta_rel<%d,%d>" % (choice[0], choice[1])
