"""The three launch cascades of the pass kernels as they stood at commit 5df326f (mgm_pass2.hip:1130-1231 with the switch of
mgm_pass2_dispatch.hip:35-48, mgm_pass.hip:269-313, mgm_pass_rel.hip:896-943), restated line by line: the arguments are what
PassParams / RelParams and the launchers' own parameters held, the answer is the instance that was launched -- as a
PassKernelChoice in field order -- or None where the cascade returned hipErrorInvalidValue.  tests/test_pass_kernel_plan.py
holds plan_dense / plan_rel (mgm_amd/csrc/mgm_planner.h) against it."""

CHOICE = "family LPL FH WEIGHTED R MGM C8 SUBV DEEP XCDQ ONEB W2 PUBE NK SPL CB FH2 lds block".split()
REFUSE, FIRST, SECOND, REL = range(4)
COMPACT_LABELS = (64, 128, 192, 256, 384, 512, 768, 1024)  # c8_supported


def choice(family, **kw):
    c = dict.fromkeys(CHOICE, 0)
    c.update(kw, family=family)
    return tuple(int(c[f]) for f in CHOICE)


def name(c):
    """The instance as a kernel trace prints it."""
    c = dict(zip(CHOICE, c))
    b = lambda v: "true" if v else "false"
    if c["family"] == FIRST:
        return "k_pass<%d, %s, %s, %d>" % (c["LPL"], b(c["FH"]), b(c["WEIGHTED"]), c["R"])
    if c["family"] == SECOND:
        return "k_pass2<%d, %s, %s, %d, %d, %d, %s, %s, %s, %s>" % (c["LPL"], b(c["FH"]), b(c["WEIGHTED"]), c["MGM"], c["C8"], c["SUBV"], b(c["DEEP"]), b(c["XCDQ"]),
                                                                 b(c["ONEB"]), b(c["W2"]))
    if c["family"] == REL:
        return "k_pass_rel<%s, %s, %d, %d, %d, %s>" % (b(c["FH"]), b(c["PUBE"]), c["NK"], c["SPL"], c["CB"], b(c["FH2"]))
    return "refused"


# ---- what the kernels report -------------------------------------------------------------------------------------------------
def pass_lpl(L):  # mgm_pass.hip
    lpl = (L + 63) // 64
    if lpl in (5, 7):
        return lpl + 1
    if lpl <= 8:
        return lpl
    return 12 if lpl <= 12 else (16 if lpl <= 16 else (24 if lpl <= 24 else 32))


def pass2_lines(L, c8):  # mgm_pass2_dispatch.hip, a default build (MGM_P2_C8_NC = 15)
    if L % 64:
        return 0
    lpl = L // 64
    if c8 and L in COMPACT_LABELS:
        return 15 if lpl <= 4 else 7
    if lpl in (1, 2, 3, 4):
        return 14
    if lpl in (6, 8, 12, 16):
        return 7
    return 0


# ---- the second build: launch_pass2 -> launch_pass2_lpl -> launch2_w2 / launch2_mgm -> launch2_one -> launch2_c8 ----------------
def launch_pass2(p, fh, wmode, dev):
    """p: L, subv, C8 (vol[0].C8 is not null), cbytes, deep, xcdq, oneb, wsel (vol[0].wsel is not null), MGM, wg_per_cu"""
    # switch (p.subv > 1 ? 4 : (p.L % 64 ? 0 : p.L / 64))
    LPL = 4 if p["subv"] > 1 else (0 if p["L"] % 64 else p["L"] // 64)
    if LPL not in (1, 2, 3, 4, 6, 8, 12, 16):
        return None  # default: return hipErrorInvalidValue

    def launch2_c8(WEIGHTED, MGM, C8, SUBV=1, DEEP=False, XCDQ=False, ONEB=False, W2=False):
        # if (p.wg_per_cu < 2 && shmem < 81 * 1024) shmem = 81 * 1024  -- the floor; the instance's own bytes stay in the kernel's unit
        return choice(SECOND, LPL=LPL, FH=fh, WEIGHTED=WEIGHTED, MGM=MGM, C8=C8, SUBV=SUBV, DEEP=DEEP, XCDQ=XCDQ, ONEB=ONEB, W2=W2,
                      lds=81 * 1024 if p["wg_per_cu"] < 2 else 0)

    def launch2_one(WEIGHTED, MGM):
        if LPL == 4 and not WEIGHTED and not (fh and MGM == 2):
            if p["subv"] > 1 and p["xcdq"]:
                return None
            if p["subv"] == 2 and p["C8"]:
                return launch2_c8(WEIGHTED, MGM, 1, 2, True) if p["deep"] else launch2_c8(WEIGHTED, MGM, 1, 2)
            if p["subv"] == 4 and p["C8"]:
                return launch2_c8(WEIGHTED, MGM, 1, 4, True) if p["deep"] else launch2_c8(WEIGHTED, MGM, 1, 4)
        if p["subv"] > 1:
            return None
        if not WEIGHTED and not (fh and MGM == 2) and LPL <= 8:
            if p["C8"] and p["cbytes"] == 2:
                if not p["deep"]:
                    return None
                if not dev:
                    if p["xcdq"] and p["oneb"]:
                        return launch2_c8(WEIGHTED, MGM, 2, 1, True, True, True)
                    if p["xcdq"]:
                        return launch2_c8(WEIGHTED, MGM, 2, 1, True, True, False)
                if p["xcdq"]:
                    return None
                return launch2_c8(WEIGHTED, MGM, 2, 1, True)
        if p["C8"] and p["cbytes"] == 2:
            return None
        if not WEIGHTED and not (fh and MGM == 2):
            if p["C8"] and p["deep"]:
                if not dev:
                    if p["xcdq"] and p["oneb"]:
                        return launch2_c8(WEIGHTED, MGM, 1, 1, True, True, True)
                    if p["xcdq"]:
                        return launch2_c8(WEIGHTED, MGM, 1, 1, True, True, False)
                if p["xcdq"]:
                    return None
                return launch2_c8(WEIGHTED, MGM, 1, 1, True)
        if p["C8"]:
            return launch2_c8(WEIGHTED, MGM, 1)
        return launch2_c8(WEIGHTED, MGM, 0)

    def launch2_mgm(WEIGHTED):
        if p["MGM"] in (1, 2, 3, 4):
            return launch2_one(WEIGHTED, p["MGM"])
        return None

    def launch2_w2():
        if LPL <= 4 and not dev:
            if not p["C8"] or not p["deep"] or not p["xcdq"] or p["subv"] > 1 or not p["wsel"]:
                return None
            if p["MGM"] in (1, 2, 3, 4):
                return launch2_c8(False, p["MGM"], 1, 1, True, True, True, True)
            return None
        return None

    # launch_pass2_lpl<MGM_P2_LPL>
    if wmode == 2:
        return launch2_w2()
    if not wmode:
        return launch2_mgm(False)
    if LPL >= 12:
        return None
    return launch2_mgm(True)


# ---- the first build: launch_pass -> launch_lpl -> launch_one ----------------------------------------------------------------------
def launch_pass(p, R, fh, wmode):
    """p: L"""
    lpl = pass_lpl(p["L"])
    WEIGHTED = bool(wmode)

    def launch_one():
        LP = lpl * 64
        NS = 2 if (WEIGHTED and not fh) else 1
        return choice(FIRST, LPL=lpl, FH=fh, WEIGHTED=WEIGHTED, R=R, lds=4 * (R * 2 * NS * LP + R * 2) + 16, block=R * 64)

    if R == 4:
        return launch_one() if lpl in (12, 16, 24, 32) else None
    if R != 16:
        return None
    return launch_one() if lpl in (1, 2, 3, 4, 6, 8) else None


# ---- the range-proportional kernels: launch_pass_rel -> launch_rel_fmt -> launch_rel_one ------------------------------------------
RR, RD4, SD = 16, 4, 8


def launch_pass_rel(p, fh, pube, wg_per_cu):
    """p: slots, cb, fh_multi, fh2, MGM, diag_any"""
    SPL = 8 if p["slots"] == 128 else 4
    CB = 4 if p["cb"] == 4 else (2 if p["cb"] == 2 else 1)

    def launch_rel_one(FH, PUBE, NK, FH2=False):
        NS = 1 if (FH or PUBE) else 2
        SLOTS = 16 * SPL
        HS = (3 * SLOTS + 2 * SPL if FH2 else (SLOTS + 2 * SPL if NS == 1 else NS * SLOTS)) + 4
        shmem = 4 * (RR * RD4 * HS + (2 if p["diag_any"] else 1) * SD * HS + 2 * SD * RR * 4) + SD * RR * SLOTS * CB + 4 * (SD + 4) + 16 + 4 * RR * 24
        if wg_per_cu >= 1:
            want = (160 * 1024) // (wg_per_cu + 1) + 1024
            if shmem < want:
                shmem = want
        return choice(REL, FH=FH, PUBE=PUBE, NK=NK, SPL=SPL, CB=CB, FH2=FH2, lds=shmem)

    if fh:
        if SPL == 4 and CB == 1:
            if not p["fh_multi"]:
                return launch_rel_one(True, False, 0)
        if p["fh2"]:
            if SPL == 8 and CB == 4:
                return None
            return launch_rel_one(True, False, 2, True)
        if p["MGM"] in (1, 2, 3):
            return launch_rel_one(True, False, p["MGM"])
        return launch_rel_one(True, False, 4)
    return launch_rel_one(False, True, 0) if pube else launch_rel_one(False, False, 0)
