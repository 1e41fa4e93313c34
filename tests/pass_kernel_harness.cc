// pass_kernel_harness.cc -- the kernel choice of plan_dense / plan_rel (mgm_amd/csrc/mgm_planner.h) behind a C interface for
// tests/test_pass_kernel_plan.py.  Built with plain g++ and no ROCm include path, like planner_harness.cc; with
// -DPASS_KERNEL_MAIN it is a stand-alone program (the sanitizer run): requests from a file in, one line per plan out.
#include <cstdio>

#include "mgm_planner.h"

using namespace mgm;

constexpr int kChoiceInts = (int)(sizeof(PassKernelChoice) / sizeof(int));
constexpr int kDenseOut = 11 + kChoiceInts, kRelOut = 3 + kChoiceInts;

extern "C" {

int pass_dense_request_ints() { return (int)(sizeof(DenseRequest) / sizeof(int)); }
int pass_rel_request_ints() { return (int)(sizeof(RelRequest) / sizeof(int)); }
int pass_choice_ints() { return kChoiceInts; }

// `n` requests as their ints, one after the other (integers only, no padding: static_assert in the header); per request
// out = err, R2, R, subv, deep, xcdq, one_queue, oneb, w2, wk, wg_per_cu, then the choice's ints
void pass_kernel_dense(const int *reqs, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        DenseRequest q;
        memcpy(&q, reqs + (size_t)i * (sizeof q / sizeof(int)), sizeof q);
        const DensePlan p = plan_dense(q);
        const int v[11] = {p.err, p.R2, p.R, p.subv, p.deep, p.xcdq, p.one_queue, p.oneb, p.w2, p.wk, p.wg_per_cu};
        memcpy(out + (size_t)i * kDenseOut, v, sizeof v);
        memcpy(out + (size_t)i * kDenseOut + 11, &p.kernel, sizeof p.kernel);
    }
}

// volumes per wave, asked before `lines2` is filled (as run_passes does)
void pass_dense_subv(const int *reqs, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        DenseRequest q;
        memcpy(&q, reqs + (size_t)i * (sizeof q / sizeof(int)), sizeof q);
        out[i] = dense_subv(q);
    }
}

// out = err, rel_wg, diag_any, then the choice's ints
void pass_kernel_rel(const int *reqs, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        RelRequest q;
        memcpy(&q, reqs + (size_t)i * (sizeof q / sizeof(int)), sizeof q);
        const RelPlan p = plan_rel(q);
        const int v[3] = {p.err, p.rel_wg, p.diag_any};
        memcpy(out + (size_t)i * kRelOut, v, sizeof v);
        memcpy(out + (size_t)i * kRelOut + 3, &p.kernel, sizeof p.kernel);
    }
}

// does the shared statement of the built instances declare this one (dev: a development build of the second build)?
void pass_kernel_exists(const int *choices, int n, int dev, int *out)
{
    for (int i = 0; i < n; i++) {
        PassKernelChoice k;
        memcpy(&k, choices + (size_t)i * kChoiceInts, sizeof k);
        out[i] = pass_instance_exists(k, dev != 0) ? 1 : 0;
    }
}

int pass_kernel_name_of(const int *choice, char *buf, int cap)
{
    PassKernelChoice k;
    memcpy(&k, choice, sizeof k);
    return pass_kernel_name(k, buf, (size_t)cap);
}

}  // extern "C"

#ifdef PASS_KERNEL_MAIN
// file: nd, nr, then nd dense requests and nr range-proportional ones as ints; one line per request: its out row, then the name
int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int head[2];
    if (!f || fread(head, sizeof(int), 2, f) != 2) return 2;
    std::vector<int> d((size_t)head[0] * pass_dense_request_ints()), r((size_t)head[1] * pass_rel_request_ints());
    if (fread(d.data(), sizeof(int), d.size(), f) != d.size() || fread(r.data(), sizeof(int), r.size(), f) != r.size()) return 2;
    fclose(f);
    std::vector<int> od((size_t)head[0] * kDenseOut), orl((size_t)head[1] * kRelOut);
    pass_kernel_dense(d.data(), head[0], od.data());
    pass_kernel_rel(r.data(), head[1], orl.data());
    auto print = [](const int *row, int nout) {
        char name[96];
        pass_kernel_name_of(row + nout - kChoiceInts, name, (int)sizeof name);
        for (int k = 0; k < nout; k++) printf("%d ", row[k]);
        printf("%s\n", name);
    };
    for (int i = 0; i < head[0]; i++) print(od.data() + (size_t)i * kDenseOut, kDenseOut);
    for (int i = 0; i < head[1]; i++) print(orl.data() + (size_t)i * kRelOut, kRelOut);
    return 0;
}
#endif
