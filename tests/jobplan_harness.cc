// jobplan_harness.cc -- plan_job and refuse_on_session (src/mgm_jobplan.h) behind a C interface for tests/test_jobplan.py.
// Built with plain g++ against that header alone: no library, no ROCm include path -- which is also the proof that a plan
// needs no device.  The environment is the dictionary the caller passes, never the process's.
#include "mgm_jobplan.h"

using namespace mgm_cli;

namespace {

struct Json {
    std::string s = "{";
    void key(const char *k) { s += (s.size() > 1 ? ",\"" : "\"") + std::string(k) + "\":"; }
    void str(const char *k, const std::string &v)
    {
        key(k);
        s += '"';
        for (unsigned char c : v) {
            char buf[8];
            if (c == '"' || c == '\\') s += '\\', s += (char)c;
            else if (c < 0x20 || c >= 0x7f) snprintf(buf, sizeof buf, "\\u%04x", c), s += buf;
            else s += (char)c;
        }
        s += '"';
    }
    void num(const char *k, long long v) { key(k), s += std::to_string(v); }
    void real(const char *k, double v)  // (as a string: a refused plan may hold a NaN)
    {
        char buf[40];
        snprintf(buf, sizeof buf, "%.17g", v);
        str(k, buf);
    }
};

JobPlan plan(const char *const *tok, int ntok, const char *const *names, const char *const *values, int nenv)
{
    return plan_job(std::vector<std::string>(tok, tok + ntok), [=](const char *name) -> const char * {
        for (int i = 0; i < nenv; i++)
            if (!strcmp(names[i], name)) return values[i];
        return nullptr;
    });
}

int give(const std::string &s, char *out, int cap)
{
    if ((int)s.size() < cap) memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}

}  // namespace

extern "C" {

// the plan of (tok, {names: values}) as one JSON object into out[cap]; returns its length (nothing is written if cap is too small)
int jobplan_plan(const char *const *tok, int ntok, const char *const *names, const char *const *values, int nenv, char *out, int cap)
{
    const JobPlan p = plan(tok, ntok, names, values, nenv);
    const Opts &o = p.o;
    Json j;
    j.str("outcome", p.outcome == JobPlan::RUN ? "run" : p.outcome == JobPlan::END ? "end" : "refuse");
    j.num("code", p.code), j.str("out", p.out_text), j.str("err", p.err_text);
    j.num("dmin", o.dmin), j.num("dmax", o.dmax), j.num("NDIR", o.NDIR), j.real("P1", o.P1), j.real("P2", o.P2), j.real("aP2", o.aP2);
    j.real("aThresh", o.aThresh), j.real("truncDist", o.truncDist), j.str("distance", o.distance), j.str("prefilter", o.prefilter);
    j.str("refine", o.refine), j.num("TSGM", o.TSGM), j.num("FH", o.FH), j.num("FIX", o.FIX), j.num("census_win", o.census_win);
    j.num("subpix", o.subpix), j.str("subpix_interp", o.subpix_interp);
    j.str("min_file", p.min_file), j.str("max_file", p.max_file), j.str("nolr_file", p.nolr_file), j.str("f_u", p.f_u), j.str("f_v", p.f_v);
    j.str("f_out", p.f_out), j.str("f_cost", p.f_cost), j.str("f_back", p.f_back), j.num("nscales", p.nscales), j.str("conf_file", p.conf_file);
    j.real("uniq", p.uniq), j.num("uniq_radius", p.uniq_radius), j.num("speckle", p.speckle), j.real("speckle_diff", p.speckle_diff);
    j.str("fill", p.fill), j.num("fill_dirs", p.fill_dirs), j.num("fill_dist", p.fill_dist), j.str("fill_occ", p.fill_occ);
    j.num("iterations", p.iterations), j.num("both", p.both), j.real("tau", p.tau), j.real("median", p.median), j.num("ranged", p.ranged);
    j.num("rfl", p.rfl), j.num("uq", p.uq), j.num("batch_lr", p.batch_lr), j.num("ms_slack", p.ms_slack), j.num("ms_radius", p.ms_radius);
    j.num("device", p.device), j.num("devices_comma", p.devices_comma), j.num("place_tries", p.place_tries);
    j.num("stats", p.stats), j.num("kernels", p.kernels), j.num("orderly_exit", p.orderly_exit);
    j.key("devices");
    j.s += "[";
    for (size_t i = 0; i < p.devices.size(); i++) j.s += (i ? "," : "") + std::to_string(p.devices[i]);
    j.s += "]}";
    return give(j.s, out, cap);
}

// refuse_on_session for the plan of the same request: {"code": ..., "err": ...}
int jobplan_refuse(const char *const *tok, int ntok, const char *const *names, const char *const *values, int nenv, int multi_up, int u_ny, int v_ny,
                   char *out, int cap)
{
    const Refusal r = refuse_on_session(plan(tok, ntok, names, values, nenv), multi_up != 0, u_ny, v_ny);
    Json j;
    j.num("code", r.code), j.str("err", r.err_text);
    j.s += "}";
    return give(j.s, out, cap);
}

}  // extern "C"
