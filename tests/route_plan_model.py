"""What decided the route of an aggregation call before the route planners existed: aggregate_batch_now (mgm_api.hip, lines 88-158 and
220-222) and resolve_dense_operands (mgm_plan.hip, lines 311-465) of commit 5fa7fa3, transcribed statement by statement.  The probes
of the device are callbacks that log their names, so a run of the model gives the decision AND the order the facts were fetched in;
tests/test_route_plan.py holds plan_agg_route, plan_subbatch, shrink_after_nomem and plan_dense_kernels (mgm_planner.h) to both."""

NEED_WEIGHTS, NEED_REL, NEED_C8, NEED_PAD = 1, 2, 3, 4  # PlanNeed
DENSE, REL = 0, 1
OK, MIXED_WEIGHTS, RAGGED_HULLS, FH2_NEEDS_SECOND_BUILD = 0, 1, 2, 3
K_CHUNK_LABELS = 32
K_MAX_LPL = 32

ROUTE_FIELDS = ("n MGM fh want_S weights_given p1_nonneg p2_nonneg p2_finite only_rel rel_enabled sw_rel sw_rel_tie sw_rel_S sw_rel_fh2 "
                "w_odd w_any").split()
ROUTE_ARRAYS = "rel_usable rel_slots rel_cb".split()
SUB_FIELDS = "npix ws_limit lr_pad route n NDIR L rel_slots want_S refine prune_enabled".split()
DENSE_FIELDS = ("nb MGM fh allow_pad Lreal p1_nonneg p2_nonneg p2_finite force_build lines_real lines_pad lpl_real lpl_pad sw_pad sw_c8 sw_deep "
                "weights_given w_given[] ragged nan_words same_hull p8_valid[] p8_L[] p8_cb[] pad_hint w_not_one[] w_odd[] w_one_other[] c8_use[] "
                "c8_bytes[] nan_found[] pad_fits[3]").split()
DENSE_OUT = "err exact first_build L padded own_padded use_c8 cb weighted weighted_given w2cand ragged fh2_ragged borrow_ones need_pad_f32 pad_hint".split()


def padded_labels(L):  # mgm_fillplan.h
    for lp in (64, 128, 192, 256, 384, 512, 768, 1024):
        if lp >= L:
            return lp
    return 0


def pass2_lines_f32(L):  # pass2_lines(L, false), mgm_pass2_dispatch.hip
    if L % 64:
        return 0
    lpl = L // 64
    if lpl in (1, 2, 3, 4):
        return 14
    if lpl in (6, 8, 12, 16):
        return 7
    return 0


def pass_lpl(L):  # mgm_pass.hip
    lpl = (L + 63) // 64
    if lpl == 5:
        return 6
    if lpl == 7:
        return 8
    if lpl <= 8:
        return lpl
    return 12 if lpl <= 12 else (16 if lpl <= 16 else (24 if lpl <= 24 else 32))


def agg_route(q, weights, rel):
    """aggregate_batch_now, lines 88-121.  q: the call and the switches; weights = (odd, any): what weights_have_odd_values would
    return; rel[v] = (usable, rel_slots, rel_cb): what rel_resolve would leave in volume v.  -> ((route, rel_weighted), probes)"""
    log = []
    n, MGM, use_fh = q["n"], q["MGM"], q["fh"]
    rel_pays = use_fh > 0 or q["weights_given"] or n >= 2 or q["only_rel"] or q["sw_rel"] >= 2 or q["sw_rel_tie"] != 0
    rel_sign_ok = bool(q["p1_nonneg"] and q["p2_nonneg"])
    rel_weighted = bool(q["weights_given"])
    rel_candidate = (not q["want_S"] or q["sw_rel_S"] != 0) and q["p2_finite"] and rel_pays and rel_sign_ok and q["rel_enabled"]
    if rel_candidate and rel_weighted:
        log.append((NEED_WEIGHTS, 0))
        odd, any_ = weights
        rel_sign_ok = not odd
        if MGM == 2 and not any_:
            rel_weighted = False
    rel_fn_ok = MGM != 2 or rel_weighted or use_fh <= 0 or q["sw_rel_fh2"] != 0
    if rel_candidate and rel_sign_ok and rel_fn_ok:
        all_ = True
        v = 0
        while v < n and all_:
            log.append((NEED_REL, v))
            u = rel[v][0]
            all_ = bool(u) and rel[v][1] == rel[0][1] and rel[v][2] == rel[0][2]
            v += 1
        if all_ and use_fh > 0 and MGM == 2 and not rel_weighted and rel[0][1] == 128 and rel[0][2] == 4:
            all_ = False
        if all_:
            return (REL, int(rel_weighted)), log
    return (DENSE, 0), log  # (the dense route decides about its weights itself)


def subbatch(route, n, npix, L, rel_slots, NDIR, ws_limit, lr_pad, want_S, ridx, prune_enabled):
    """The first chunk: lines 124-127 (range-proportional) and 147-158 (dense)."""
    chunk = n
    if route == REL:
        per_vol = 4.0 * (float(npix) * rel_slots + float(lr_pad)) * NDIR * 1.16
        if ws_limit:
            while chunk > 1 and per_vol * chunk > float(ws_limit):
                chunk -= 1
        return chunk
    if ws_limit:
        Lk = padded_labels(L) if padded_labels(L) else L
        per_vol = 4.0 * (float(npix) * Lk + float(lr_pad)) * NDIR * (1.07 + ((1.0 / K_CHUNK_LABELS) if (L == 256 and not want_S and ridx <= 1 and prune_enabled) else 0.0))
        while chunk > 1 and per_vol * chunk > float(ws_limit):
            chunk -= 1
        if chunk >= 4:
            chunk -= chunk % 4
        elif chunk == 3:
            chunk = 2
    return chunk


def shrink(route, m):
    """After MGM_ERR_NOMEM at m > 1 volumes: line 132 (range-proportional), 221-222 (dense)."""
    if route == REL:
        return max(1, m // 2)
    chunk = (m // 2) - (m // 2) % 2 if m > 4 else m // 2
    return max(chunk, 1)


def dense_kernels(q, weight_words, c8, pad_fits):
    """resolve_dense_operands.  q: the call, the volumes' host-side state and the switches; weight_words[v] = (some != 1, odd, lo == hi)
    from scan_weights' four words; c8[v] = (use, cbytes, nan_state == Invalid) after c8_resolve; pad_fits[tb]: the read-back of a pad
    try at tb bytes was 0.  -> (DENSE_OUT as a tuple, probes)"""
    log = []
    o = dict(err=OK, exact=0, first_build=0, L=0, padded=0, own_padded=0, use_c8=1, cb=1, weighted=0, weighted_given=0, w2cand=0, ragged=0, fh2_ragged=0,
             borrow_ones=0, need_pad_f32=0, pad_hint=-1)

    def done():
        return tuple(int(o[k]) for k in DENSE_OUT), log

    def refuse(err):
        return (err, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, -1), log

    nb, MGM, fh, Lreal = q["nb"], q["MGM"], bool(q["fh"]), q["Lreal"]
    first_build = o["first_build"] = q["force_build"] == 1 or not q["p1_nonneg"] or not q["p2_nonneg"]
    L = Lreal
    padded = False
    if q["allow_pad"] and not first_build and pass2_lines_f32(Lreal) == 0 and q["sw_pad"] and not (q["weights_given"] and Lreal > 512):
        lp = padded_labels(Lreal)
        if lp:
            L = lp
            padded = True
    o["L"], o["padded"] = L, padded
    lpl = pass_lpl(L)
    weighted = w2cand = wodd = False
    if q["weights_given"]:
        log.append((NEED_WEIGHTS, 0))
        w2cand = True
        for v in range(nb):
            not_one, odd, one_other = weight_words[v]
            wv = bool(q["w_given"][v] and not_one)
            if v and wv != weighted and (MGM == 2 or not q["w_given"][v]):
                return refuse(MIXED_WEIGHTS)
            weighted = weighted or wv
            wodd = wodd or (wv and bool(odd))
            w2cand = w2cand and (not wv or (not odd and bool(one_other)))
        w2cand = w2cand and weighted
    o["weighted_given"] = weighted
    ragged = o["ragged"] = bool(q["ragged"])
    o["exact"] = (ragged and not q["p2_finite"]) or Lreal > K_MAX_LPL * 64 or (ragged and fh and (not q["p1_nonneg"] or wodd))
    o["exact"] = o["exact"] or bool(q["nan_words"])
    if o["exact"]:
        return done()
    if fh and ragged and not q["same_hull"]:
        return refuse(RAGGED_HULLS)
    if fh and ragged and not weighted:
        o["fh2_ragged"] = MGM == 2
        if o["fh2_ragged"] and (first_build or pass2_lines_f32(L) == 0):
            return refuse(FH2_NEEDS_SECOND_BUILD)
        o["borrow_ones"] = 1  # (reserve + upload of c->ones8)
        weighted = True
    o["weighted"], o["w2cand"] = weighted, w2cand
    use_c8 = True
    c8ok = [0] * nb
    for v in range(nb):
        log.append((NEED_C8, v))
        c8ok[v] = c8[v][0]
        o["exact"] = o["exact"] or bool(c8[v][2])
    if o["exact"]:
        return done()
    cb = 1
    own_padded = bool(padded and q["sw_c8"])
    v = 0
    while v < nb and own_padded:
        own_padded = bool(q["p8_valid"][v]) and q["p8_L"][v] == L and q["p8_cb"][v] == q["p8_cb"][0]
        v += 1
    if own_padded:
        cb = q["p8_cb"][0]
    elif padded:
        tries = [2 if q["pad_hint"] == 2 else 1, 1 if q["pad_hint"] == 2 else 2, 0]
        if q["pad_hint"] == 0:
            tries[0] = 0
        use_c8 = False
        t = 0
        while t < 3 and q["sw_c8"] and not use_c8:
            tb = tries[t]
            if tb == 0 or (tb == 2 and L > 512):
                break
            log.append((NEED_PAD, tb))
            if pad_fits[tb]:
                use_c8 = True
                cb = tb
            t += 1
        o["pad_hint"] = cb if use_c8 else 0
        if not use_c8:
            o["need_pad_f32"] = 1
    else:
        for v in range(nb):
            use_c8 = use_c8 and bool(c8ok[v]) and c8[v][1] == c8[0][1]
        cb = c8[0][1] if use_c8 else 1
    if use_c8 and cb == 2 and (weighted or (fh and MGM == 2) or lpl > 8 or q["sw_deep"] == 0):
        own_padded = False
        if padded:
            o["need_pad_f32"] = 1
        use_c8 = False
    if first_build or (weighted and lpl > 8):
        use_c8 = False
    o["use_c8"], o["cb"], o["own_padded"] = use_c8, cb, own_padded
    return done()
