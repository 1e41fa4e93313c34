"""The tag protocol of the self-validating hand-off slots as run_passes / run_rel (mgm_amd/csrc/mgm_plan.hip) and mgm_ctx.hip wrote
it INLINE at commit 098beb7, restated for tests/test_hand_tags.py: the dense region (hand_key, hand_tags[8]) and the
range-proportional one (hand_rel_key, hand_rel_tag); and a simulated region that knows which tags a slot may carry.

Events are tuples (kind, region, layout, first, count, moved, fails): LAUNCH of the passes [first, first + count) on a region laid
out as `layout` (an index; two layouts are equal iff their indices are), whose buffer moved or not, and which fails before its kernel
is enqueued or not; WATCHDOG: the context finds the sticky watchdog word set -- the launch enqueued last timed out; TRIM."""
LAUNCH, WATCHDOG, TRIM = 0, 1, 2
DENSE, REL = 0, 1
NPASS = 8
TAG = 0x80000000
CLEARED = TAG  # the tag bit of a cleared (all-ones) word


class Parent:
    """Both inline versions.  run(events) -> per event None, or (clear, {pass: tag handed to the kernel})."""

    def __init__(self):
        self.hand_key, self.hand_tags = None, [0] * NPASS  # (None: HandLayout{}, which equals no layout of a launch)
        self.hand_rel_key, self.hand_rel_tag = None, 0

    def launch_dense(self, layout, first, count, moved, fails):  # mgm_plan.hip:480-498, 603
        clear = moved or self.hand_key != layout
        if clear:
            self.hand_key = layout
            self.hand_tags = [TAG] * NPASS
        handed = {}
        for k in range(first, first + count):
            self.hand_tags[k] ^= TAG
            handed[k] = self.hand_tags[k]
        self.hand_key = None
        if not fails:
            self.hand_key = layout
        return clear, handed

    def launch_rel(self, layout, first, count, moved, fails):  # mgm_plan.hip:912-926, 977 (one tag for the passes [0, NDIR))
        clear = moved or self.hand_rel_key != layout
        if clear:
            self.hand_rel_key = layout
            self.hand_rel_tag = TAG
        self.hand_rel_tag ^= TAG
        self.hand_rel_key = None
        if not fails:
            self.hand_rel_key = layout
        return clear, {k: self.hand_rel_tag for k in range(first, first + count)}

    def watchdog(self):  # mgm_ctx.hip:160 -- the dense region alone
        self.hand_key = None

    def trim(self):  # mgm_ctx.hip:266, 278
        self.hand_key = self.hand_rel_key = None

    def run(self, events):
        out = []
        for kind, region, layout, first, count, moved, fails in events:
            if kind == LAUNCH:
                out.append((self.launch_rel if region == REL else self.launch_dense)(layout, first, count, bool(moved), bool(fails)))
            else:
                self.watchdog() if kind == WATCHDOG else self.trim()
                out.append(None)
        return out


def violations(events, steps):
    """The protocol's invariant against simulated regions: [(event index, pass, tag)] of the launches that hand a pass a tag which a
    slot of that pass may still carry.  may[region][pass] = the tags its slots may carry: CLEARED, the tag of the last launch that
    wrote them all, both after a launch that timed out; every tag once the buffer moved (fresh memory) or the slots are laid out for
    another layout than the launch's (a pass's slots then overlap other passes' old ones) -- until somebody clears the region."""
    anything = {0, TAG}
    may = [[set(anything) for _ in range(NPASS)] for _ in (DENSE, REL)]
    laid = [None, None]
    last = None  # (region, {pass: tags before it}, handed) of the launch enqueued last, until the watchdog has spoken of it
    bad = []
    for i, (ev, step) in enumerate(zip(events, steps)):
        kind, region, layout, first, count, moved, fails = ev
        if kind == WATCHDOG:
            if last:
                r, before, handed = last
                for k, t in handed.items():
                    may[r][k] = before[k] | {t}
            last = None
            continue
        if kind == TRIM:
            may = [[set(anything) for _ in range(NPASS)] for _ in (DENSE, REL)]
            laid, last = [None, None], None
            continue
        clear, handed = step
        if moved or laid[region] != layout:
            may[region] = [set(anything) for _ in range(NPASS)]
        if clear:
            may[region] = [{CLEARED} for _ in range(NPASS)]
        if clear or laid[region] != layout:
            laid[region] = layout
        assert sorted(handed) == list(range(first, first + count)), (i, ev, handed)
        bad += [(i, k, t) for k, t in handed.items() if t in may[region][k]]
        if not fails:
            last = (region, {k: set(may[region][k]) for k in handed}, dict(handed))
            for k, t in handed.items():
                may[region][k] = {t}
    return bad
