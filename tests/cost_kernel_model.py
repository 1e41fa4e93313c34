"""Which K2 kernel fills a cost volume, as the launchers decided it before plan_cost_kernel (mgm_fillplan.h) existed: launch_cost
(mgm_cost.hip) and launch_cost_fast (mgm_cost_fast.hip) of commit c0ec791, restated branch by branch over arrays of requests --
the predicate of each kernel family in the cascade's order, the grid arithmetic with its caps, floors and `+ 1`s, the LDS bytes,
the template switch with the `default:` arms it had, the name string from its nested ternaries, the refusal of a padded layout no
restructured kernel took.  Written from that commit, not from the planner, which tests/test_cost_kernel_plan.py holds against it.

A request is what the cascade read of CostParams: costfn, nch, the two image sizes, L (the slots of the layout), Lreal, cbytes,
hwin, trunc, and four pointers as flags -- p.C (`f32`), p.C8 (`compact`), p.rlo (`ragged`), p.ncc_u && p.ncc_v (`scratch`).
The answer: the family, the template arguments of the instance (0 where the family has none), the kernel that ran on both images
first with its two grids, the grid, the dynamic LDS bytes, the census truncation byte, and the name in the timing table."""
import numpy as np

FIELDS = "costfn nch nx ny vnx vny L Lreal cbytes hwin f32 compact ragged scratch".split()
OUT = "family FN W4 CB SD NCH LN HW pre pre_grid_u pre_grid_v grid lds tb".split()
REFUSED, NCC, BTX_BT, BTX_DIFF, BTX_CENSUS, DIFFX, CENSUS8X, CENSUS8, GENERAL = range(9)
FAMILIES = "refused k_cost_ncc k_cost_btx(bt) k_cost_btx(diff) k_cost_btx(census) k_cost_diffx k_cost_census8x k_cost_census8 k_cost".split()
PRE_NONE, PRE_NCC_STATS, PRE_BT_SPANS = range(3)
NAME_BYTES = 24
COMPACT_LABELS = (64, 128, 192, 256, 384, 512, 768, 1024)  # c8_supported
NCC_PXB, NCC_MAX_HW, NCC_MAX_L = 32, 3, 1024                # kNccPxb, kNccMaxHw, kNccMaxL


def u32(x):
    return x & 0xffffffff  # (unsigned)(a long long)


def float_to_unsigned(t):
    """(unsigned)p.trunc as the host code computes it: the low 32 bits of the float's truncation to a 64-bit integer, which is
    what the language defines for -1 < t < 2^32 and what x86-64 does beyond (a NaN converts to 0x8000000000000000: 0)."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        whole = np.where(np.isfinite(t), np.trunc(t), 0.0).astype(np.int64)
    return u32(whole)


def choose(req, trunc):
    """req: integers [n][len(FIELDS)], trunc: float32 [n] -> (integers [n][len(OUT)], names [n] as bytes)."""
    req, trunc = np.asarray(req, np.int64), np.asarray(trunc, np.float32)
    n = len(req)
    q = {f: req[:, k] for k, f in enumerate(FIELDS)}
    costfn, nch, nx, ny, vnx, vny, L, Lreal, cbytes, hwin = (q[f] for f in FIELDS[:10])
    C, C8, rlo, ncc = q["f32"] != 0, q["compact"] != 0, q["ragged"] != 0, q["scratch"] != 0
    out = np.zeros((n, len(OUT)), np.int64)
    o = {f: out[:, k] for k, f in enumerate(OUT)}
    names = np.full(n, b"k_cost_general", "S%d" % NAME_BYTES)
    npix, vpix = nx * ny, vnx * vny
    w4 = nx % 4 == 0
    c8_supported = np.isin(L, COMPACT_LABELS)
    left = np.ones(n, bool)  # the requests no branch above has returned from

    # if (p.costfn == 3 && p.ncc_u && p.ncc_v && p.C && !p.C8 && !p.rlo && p.hwin >= 1 && p.hwin <= kNccMaxHw && p.L <= kNccMaxL && p.nch <= 4)
    m = left & (costfn == 3) & ncc & C & ~C8 & ~rlo & (hwin >= 1) & (hwin <= NCC_MAX_HW) & (L <= NCC_MAX_L) & (nch <= 4)
    o["family"][m], o["pre"][m] = NCC, PRE_NCC_STATS
    o["pre_grid_u"][m], o["pre_grid_v"][m] = u32((npix[m] + 255) // 256), u32((vpix[m] + 255) // 256)
    win = 2 * hwin[m] + 1
    o["lds"][m] = 4 * nch[m] * win * ((NCC_PXB + 2 * hwin[m]) + (NCC_PXB + L[m] - 1 + 2 * hwin[m]))
    o["grid"][m] = u32(((nx[m] + NCC_PXB - 1) // NCC_PXB) * ny[m])
    o["HW"][m] = np.where(hwin[m] == 1, 1, np.where(hwin[m] == 2, 2, 3))  # switch (p.hwin) { case 1: case 2: default: k_cost_ncc<3> }
    names[m] = b"k_cost_ncc"
    left &= ~m

    nw = ((nx + 3) // 4 * ny + 3) // 4  # k_cost_btx: if (nw > 256 * 64) nw = 256 * 64; if (nw < 1) nw = 1;
    nw = np.maximum(np.minimum(nw, 256 * 64), 1)
    # if (p.costfn >= 4 && p.ncc_u && p.ncc_v && p.C && !p.C8 && !p.rlo && p.L % 4 == 0)
    m = left & (costfn >= 4) & ncc & C & ~C8 & ~rlo & (L % 4 == 0)
    o["family"][m], o["pre"][m] = BTX_BT, PRE_BT_SPANS
    o["pre_grid_u"][m], o["pre_grid_v"][m] = u32((npix[m] * nch[m] + 255) // 256), u32((vpix[m] * nch[m] + 255) // 256)
    o["grid"][m] = nw[m]
    o["FN"][m] = np.where(costfn[m] == 5, 5, 4)  # if (p.costfn == 5) launch_btx<5> else launch_btx<4>
    o["W4"][m] = w4[m]
    names[m] = np.where(w4[m], b"k_cost_btx_bt_w4", b"k_cost_btx_bt")
    left &= ~m

    # if (p.costfn <= 2 && p.C && !p.C8 && !p.rlo && p.L % 4 == 0)
    m = left & (costfn <= 2) & C & ~C8 & ~rlo & (L % 4 == 0)
    o["family"][m] = np.where(costfn[m] == 2, BTX_CENSUS, BTX_DIFF)
    o["grid"][m] = nw[m]
    o["FN"][m] = np.where(costfn[m] == 0, 0, np.where(costfn[m] == 1, 1, 2))
    o["W4"][m] = w4[m]
    names[m] = np.where(costfn[m] == 2, np.where(w4[m], b"k_cost_btx_census_w4", b"k_cost_btx_census"), np.where(w4[m], b"k_cost_btx_diff_w4", b"k_cost_btx_diff"))
    left &= ~m

    # if (!p.C && p.C8 && (p.costfn == 0 || p.costfn == 1) && !p.rlo && npix < 0x7fffffffll && c8_supported(p.L) &&
    #     (p.cbytes == 1 || p.cbytes == 2) && p.L * p.cbytes <= 1024 && p.trunc >= 0.0f && !__builtin_signbit(p.trunc))
    with np.errstate(invalid="ignore"):
        tpos = (trunc >= 0) & ~np.signbit(trunc)
    m = left & ~C & C8 & ((costfn == 0) | (costfn == 1)) & ~rlo & (npix < 0x7fffffff) & c8_supported & ((cbytes == 1) | (cbytes == 2)) & (L * cbytes <= 1024) & tpos
    o["family"][m] = DIFFX
    # launch_diffx: nw = ((nx + 3) / 4 * ny * 4 * L * CB / 4096 + 3) / 4 + 1; if (nw > 256 * 32) nw = 256 * 32;
    o["grid"][m] = np.minimum(((nx[m] + 3) // 4 * ny[m] * 4 * L[m] * cbytes[m] // 4096 + 3) // 4 + 1, 256 * 32)
    o["CB"][m], o["SD"][m] = cbytes[m], costfn[m] == 1
    spec = (nch[m] == 1) | (nch[m] == 3)
    o["NCH"][m] = np.where(spec, nch[m], 0)  # if (p.nch == 1) <CB, 1, SD> else if (p.nch == 3) <CB, 3, SD> else <CB, 0, SD>
    names[m] = np.where(cbytes[m] == 2, np.where(spec, b"k_cost_diffx_2b", b"k_cost_diffx_2b_anych"), np.where(spec, b"k_cost_diffx_1b", b"k_cost_diffx_1b_anych"))
    left &= ~m

    # if (!p.C && p.C8 && p.costfn == 2 && p.nch == 1 && c8_supported(p.L))
    m = left & ~C & C8 & (costfn == 2) & (nch == 1) & c8_supported
    o["tb"][m] = np.where(np.isposinf(trunc[m]), 255, float_to_unsigned(trunc[m]))
    x = m & (npix < 0x7fffffff)  # if (npix < 0x7fffffffll) { ... k_cost_census8x ...; return }
    o["family"][x] = CENSUS8X
    o["grid"][x] = np.minimum(((nx[x] + 3) // 4 * ny[x] * 4 * L[x] // 4096 + 3) // 4 + 1, 256 * 32)
    o["LN"][x] = np.where(np.isin(L[x], COMPACT_LABELS[:-1]), L[x], 1024)  # switch (p.L) { case 64: ... default: launch_census8x<1024> }
    o["W4"][x] = w4[x]
    names[x] = np.where(w4[x], b"k_cost_census8x_w4", b"k_cost_census8x")
    # (k_cost_census8w: behind `npix < 0x7fffffffll` in the fall-through of the test above -- taken by no request)
    y = m & ~x
    o["family"][y] = CENSUS8
    o["grid"][y] = u32(np.minimum((npix[y] + 3) // 4, 256 * 32))
    o["LN"][y] = np.where(np.isin(L[y] // 64, (1, 2, 3, 4, 6, 8, 12)), L[y] // 64, 16)  # switch (p.L / 64) { ... default: k_cost_census8<16> }
    names[y] = b"k_cost_census8"
    left &= ~m

    # launch_cost: *which = "k_cost_general"; if (p.Lreal != p.L) return hipErrorInvalidValue; k_cost on (npix + 3) / 4 workgroups
    g = left & (Lreal == L)
    o["family"][g] = GENERAL
    o["grid"][g] = u32((npix[g] + 3) // 4)
    o["family"][left & ~g] = REFUSED
    return out, names


# The instances the two launchers could launch: every template argument list of their switches (k_cost_census8w excluded: dead).
INSTANCES = ([(NCC, 0, 0, 0, 0, 0, 0, hw) for hw in (1, 2, 3)] + [(BTX_BT, fn, w, 0, 0, 0, 0, 0) for fn in (4, 5) for w in (0, 1)] +
             [(BTX_DIFF, fn, w, 0, 0, 0, 0, 0) for fn in (0, 1) for w in (0, 1)] + [(BTX_CENSUS, 2, w, 0, 0, 0, 0, 0) for w in (0, 1)] +
             [(DIFFX, 0, 0, cb, sd, c, 0, 0) for cb in (1, 2) for sd in (0, 1) for c in (1, 3, 0)] +
             [(CENSUS8X, 0, w, 0, 0, 0, L, 0) for L in COMPACT_LABELS for w in (0, 1)] + [(CENSUS8, 0, 0, 0, 0, 0, L // 64, 0) for L in COMPACT_LABELS] +
             [(GENERAL, 0, 0, 0, 0, 0, 0, 0)])
