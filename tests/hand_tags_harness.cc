// hand_tags_harness.cc -- HandTags (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_hand_tags.py.  Built with
// plain g++ and no ROCm include path, like route_plan_harness.cc.  The two regions of a context are DRIVEN here the way
// mgm_plan.hip / mgm_ctx.hip drive them: a launch begins (begin_hand), commits unless it fails before the kernel is enqueued,
// and a watchdog error or a trim forgets both regions (forget_hand_regions).
// -DHAND_TAGS_MAIN: a program of its own that runs pseudo-random sequences through the same entry point (for the sanitizers).
#include "mgm_planner.h"

using namespace mgm;

enum { kLaunch = 0, kWatchdog = 1, kTrim = 2 };
enum { kEventInts = 7, kLayoutInts = 8, kOutWords = 1 + kMaxDirs };

// desc[kLayoutInts] = nx, ny, npass, groups, slot_floats, slots, R, bands of the last pass (the others: 3)
static HandLayout make_layout(const int *d)
{
    PassGeom g[kMaxDirs] = {};
    for (int q = 0; q < d[2]; q++) g[q].nbands = q == d[2] - 1 ? d[7] : 3, g[q].LL = 5 + q, g[q].slope = q & 1;
    return lay_out_hand(g, d[2], d[0], d[1], d[3], d[4], d[5], d[6]);
}

extern "C" {

int hand_max_dirs() { return kMaxDirs; }
unsigned hand_tag_bit() { return kHandTagBit; }
int hand_clear_byte() { return kHandClearByte; }

// events[n][kEventInts] = kind, region (0 dense, 1 range-proportional), layout, first, count, moved, fails before the enqueue;
// out[n][kOutWords] = per launch: clear, the tags handed to the kernel (other events: zeros)
void hand_run(const int *layouts, int nlayouts, const int *events, int n, unsigned *out)
{
    HandTags region[2];
    for (int i = 0; i < n; i++) {
        const int *e = events + (size_t)i * kEventInts;
        unsigned *o = out + (size_t)i * kOutWords;
        memset(o, 0, sizeof(unsigned) * kOutWords);
        if (e[0] != kLaunch) {
            hand_forget(region[0]);
            hand_forget(region[1]);
            continue;
        }
        if (e[1] < 0 || e[1] > 1 || e[2] < 0 || e[2] >= nlayouts) continue;
        const HandLayout want = make_layout(layouts + (size_t)e[2] * kLayoutInts);
        const HandStep s = hand_begin(region[e[1]], want, e[3], e[3] + e[4], e[5] != 0);
        o[0] = s.clear ? 1u : 0u;
        memcpy(o + 1, s.tag, sizeof s.tag);
        if (!e[6]) hand_commit(region[e[1]], want);
    }
}

}  // extern "C"

#ifdef HAND_TAGS_MAIN
#include <cstdio>
int main()
{
    const int layouts[3][kLayoutInts] = {{160, 130, 8, 1, 256, 0, 8, 3}, {160, 130, 8, 1, 256, 0, 8, 4}, {150, 110, 4, 2, 72, 64, 4, 3}};
    unsigned long long rng = 12345, sum = 0;
    auto next = [&](int m) { return (int)((rng = rng * 6364136223846793005ULL + 1442695040888963407ULL) >> 33) % m; };
    for (int seq = 0; seq < 2000; seq++) {
        int ev[64][kEventInts];
        unsigned out[64][kOutWords];
        for (auto &e : ev) {
            const int kind = next(8), lay = next(3), npass = layouts[lay][2], first = next(npass);
            const int v[kEventInts] = {kind < 6 ? kLaunch : kind - 5, next(2), lay, first, 1 + next(npass - first), next(5) == 0, next(6) == 0};
            memcpy(e, v, sizeof v);
        }
        hand_run(&layouts[0][0], 3, &ev[0][0], 64, &out[0][0]);
        for (auto &o : out)
            for (unsigned w : o) sum = sum * 31 + w;
    }
    printf("hand_tags_harness: 2000 sequences, checksum %016llx\n", sum);
    return 0;
}
#endif
