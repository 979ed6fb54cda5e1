// Driver of `make host-oneshot-asan`: calls the real entry points of the one-shot units (gpt_batch_host.hip, gpt_batch_opt_host.hip, gpt_fold_scan_host.hip, gpt_select_host.hip,
// gpt_svgp_train_host.hip, gpt_svgp_surface_host.hip), gpt_predict_all (gpt_api.hip), gpt_inverse_map, gpt_transport_policy and
// gpt_pullback_policy (gpt_transport_host.hip), gpt_pullback_chain (gpt_chain_host.hip), gpt_rollout_policy (gpt_rollout_host.hip), gpt_rollout_stabilised (gpt_rollout_stab_host.hip), gpt_rollout_sampled (gpt_rollout_sampled_host.hip),
// gpt_rollout_pathwise (gpt_rollout_pathwise_host.hip), gpt_apply_inverse (gpt_api.hip)
// on the stand-in "device" memory of host_stub/, at the smallest shapes at which each piece of their packing, carving and sizing arithmetic can go wrong.  Every
// array is allocated at its exact size, so AddressSanitizer sees a read or write past it; every output starts as a sentinel.
// The stand-in launchers (stub_launchers.cpp) write zeros where the kernels write, so after a call an output that was asked for
// holds zeros from end to end, and one that was not, or that belongs to a failed member or a failed call, still holds the
// sentinel.  After every call nothing allocated may be left (stub_live_objects); after a call on a handle, nothing but what the
// handle held before it.  One line per case, then ONESHOT_DRIVER_OK.
#include <hip/hip_runtime.h>
#include "../../../include/gpt_hip.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace gpt {
extern int stub_fail_model;      // stub_launchers.cpp
extern bool stub_fail_flag;
extern int stub_opt_launches, stub_opt_launch_count;
extern int stub_fail_surrogate;
extern int stub_rollout_launch_count;
}

namespace {

constexpr double SENT = -7.25e300;
constexpr int ISENT = -77;

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            fprintf(stderr, "FAILED %s: %s (line %d; last error: %s)\n", g_case.c_str(), #cond, __LINE__, gpt_last_error()); \
            exit(1);                                                                                                  \
        }                                                                                                             \
    } while (0)

std::string g_case;
int g_cases = 0;

// An array of exactly n elements (n = 0 included: still a pointer of its own).
template <class T> struct Arr {
    size_t n;
    T* p;
    Arr(size_t n_, T v) : n(n_), p(new T[n_]) { std::fill(p, p + n, v); }
    Arr(std::initializer_list<T> l) : n(l.size()), p(new T[l.size()]) { std::copy(l.begin(), l.end(), p); }
    Arr(const Arr& o) : n(o.n), p(new T[o.n]) { std::copy(o.p, o.p + n, p); }
    Arr& operator=(const Arr&) = delete;
    ~Arr() { delete[] p; }
    bool all(T v, size_t b, size_t e) const { return std::all_of(p + b, p + e, [v](T x) { return x == v; }); }
    bool all(T v) const { return all(v, 0, n); }
    bool same(const Arr& o) const { return n == o.n && std::equal(p, p + n, o.p); }
};
using D = Arr<double>;

// inputs: finite, positive, distinct enough that no check refuses them
D ramp(size_t n, double first = 0.25, double step = 0.125) {
    D a(n, 0.0);
    for (size_t i = 0; i < n; ++i) a.p[i] = first + step * (double)(i % 17);
    return a;
}

void begin(const std::string& name) { g_case = name; }
void done(int rc, int want) {
    CHECK(rc == want);
    CHECK(stub_live_objects == 0);
    printf("ok  %s\n", g_case.c_str());
    ++g_cases;
}

// ---- batch --------------------------------------------------------------------------------------------------------------------
struct BatchShape {
    std::vector<int> n;
    int Dm, n_ls, O;
    int64_t B() const { return (int64_t)n.size(); }
    std::string name() const {
        std::string s = "B=" + std::to_string(B()) + " n={";
        for (int v : n) s += std::to_string(v) + ",";
        return s + "} D=" + std::to_string(Dm) + " n_ls=" + std::to_string(n_ls) + " O=" + std::to_string(O);
    }
};

struct BatchInputs {
    Arr<int64_t> n_begin, l_begin;
    D ls, c, noise;
    explicit BatchInputs(const BatchShape& s)
        : n_begin(s.n.size() + 1, 0), l_begin(s.n.size() + 1, 0), ls(ramp(s.n.size() * s.n_ls, 0.5)), c(ramp(s.n.size(), 1.0)),
          noise(ramp(s.n.size(), 0.01, 0.01)) {
        for (size_t b = 0; b < s.n.size(); ++b) { n_begin.p[b + 1] = n_begin.p[b] + s.n[b]; l_begin.p[b + 1] = l_begin.p[b] + s.n[b] * s.n[b]; }
    }
};

// slices [begin[b] * width, begin[b + 1] * width) hold zeros for a member that ran and the sentinel for the failed one
void check_slices(const D& out, const Arr<int64_t>& begin, size_t width, int failed) {
    for (size_t b = 0; b + 1 < begin.n; ++b)
        CHECK(out.all((int)b == failed ? SENT : 0.0, (size_t)begin.p[b] * width, (size_t)begin.p[b + 1] * width));
}
void check_status(const Arr<int>& status, int failed) {
    for (size_t b = 0; b < status.n; ++b) CHECK(status.p[b] == ((int)b == failed ? GPT_E_NOT_PD : GPT_OK));
}

void batch_cases(const BatchShape& s, const std::vector<int>& queries, int failed) {
    const int64_t B = s.B();
    BatchInputs in(s);
    const size_t rows = (size_t)in.n_begin.p[B];
    D X = ramp(rows * s.Dm), Y = ramp(rows * s.O);
    Arr<int64_t> one_each(B + 1, 0);
    for (int64_t b = 0; b <= B; ++b) one_each.p[b] = b;
    const std::string tag = s.name() + (failed >= 0 ? " failed=" + std::to_string(failed) : "");
    gpt::stub_fail_model = failed;
    {
        begin("gpt_batch_lml_objective " + tag);
        D lml(B, SENT), grad(B * (2 + s.n_ls), SENT);
        Arr<int> status(B, ISENT);
        done(gpt_batch_lml_objective(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, in.ls.p, s.n_ls, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, lml.p,
                                     grad.p, status.p), GPT_OK);
        check_status(status, failed);
        check_slices(lml, one_each, 1, failed);
        check_slices(grad, one_each, 2 + s.n_ls, failed);
    }
    for (int mask : {0, 3, 1, 2}) {                                      // neither optional output, both, L alone, lml alone
        begin("gpt_batch_fit " + tag + (mask & 1 ? " L" : " L=NULL") + (mask & 2 ? " lml" : " lml=NULL"));
        D L((size_t)in.l_begin.p[B], SENT), alpha(rows * s.O, SENT), lml(B, SENT);
        Arr<int> status(B, ISENT);
        done(gpt_batch_fit(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, in.ls.p, s.n_ls, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_MATERN32,
                           mask & 1 ? L.p : nullptr, alpha.p, mask & 2 ? lml.p : nullptr, status.p), GPT_OK);
        check_status(status, failed);
        check_slices(alpha, in.n_begin, s.O, failed);
        if (mask & 1) check_slices(L, in.l_begin, 1, failed);
        else CHECK(L.all(SENT));
        if (mask & 2) check_slices(lml, one_each, 1, failed);
        else CHECK(lml.all(SENT));
    }
    Arr<int64_t> q_begin(B + 1, 0);
    for (int64_t b = 0; b < B; ++b) q_begin.p[b + 1] = q_begin.p[b] + queries[b];
    const size_t M = (size_t)q_begin.p[B];
    D Xq = ramp(M * s.Dm);
    const size_t widths[5] = {(size_t)s.O, 1, (size_t)s.O * s.Dm, (size_t)s.Dm, (size_t)s.Dm};
    for (int mask : {31, 1, 2, 4, 8, 16}) {
        begin("gpt_batch_predict " + tag + " M=" + std::to_string(M) + " outputs=" + std::to_string(mask));
        std::vector<D> out;
        double* ptr[5];
        for (int k = 0; k < 5; ++k) out.emplace_back(M * widths[k], SENT);
        for (int k = 0; k < 5; ++k) ptr[k] = (mask >> k & 1) ? out[k].p : nullptr;
        Arr<int> status(B, ISENT);
        done(gpt_batch_predict(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, in.ls.p, s.n_ls, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF,
                               M ? Xq.p : nullptr, q_begin.p, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], status.p), GPT_OK);
        check_status(status, failed);
        for (int k = 0; k < 5; ++k) {
            if (ptr[k]) check_slices(out[k], q_begin, widths[k], failed);
            else CHECK(out[k].all(SENT));
        }
    }
    gpt::stub_fail_model = -1;
}

void batch_refusals() {
    BatchShape s{{1, 32, 33}, 3, 3, 3};
    BatchInputs in(s);
    D X = ramp(66 * 3), Y = ramp(66 * 3), lml(3, SENT), grad(3 * 5, SENT), alpha(66 * 3, SENT), Xq = ramp(3 * 3), mean(3 * 3, SENT);
    Arr<int> status(3, ISENT);
    Arr<int64_t> q_begin{0, 1, 2, 3};
    auto objective = [&](const double* x, const int64_t* nb, int64_t B, int Dm, int n_ls) {
        return gpt_batch_lml_objective(0, x, Y.p, nb, B, Dm, 3, in.ls.p, n_ls, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, lml.p, grad.p, status.p);
    };
    begin("gpt_batch_lml_objective refuses X = NULL"); done(objective(nullptr, in.n_begin.p, 3, 3, 3), GPT_E_ARG);
    begin("gpt_batch_lml_objective refuses B = 0"); done(objective(X.p, in.n_begin.p, 0, 3, 3), GPT_E_ARG);
    begin("gpt_batch_lml_objective refuses D = 16"); done(objective(X.p, in.n_begin.p, 3, 16, 1), GPT_E_ARG);
    Arr<int64_t> too_many{0, 129};
    D X129 = ramp(129 * 3), Y129 = ramp(129 * 3);
    begin("gpt_batch_fit refuses n_b = 129");
    done(gpt_batch_fit(0, X129.p, Y129.p, too_many.p, 1, 3, 3, in.ls.p, 3, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, nullptr, alpha.p, nullptr,
                       status.p), GPT_E_ARG);
    begin("gpt_batch_fit refuses alpha = NULL");
    done(gpt_batch_fit(0, X.p, Y.p, in.n_begin.p, 3, 3, 3, in.ls.p, 3, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, nullptr, nullptr, nullptr,
                       status.p), GPT_E_ARG);
    begin("gpt_batch_predict refuses q_begin = NULL");
    done(gpt_batch_predict(0, X.p, Y.p, in.n_begin.p, 3, 3, 3, in.ls.p, 3, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, Xq.p, nullptr, mean.p, nullptr,
                           nullptr, nullptr, nullptr, status.p), GPT_E_ARG);
    begin("gpt_batch_predict refuses J of a Matern batch");
    done(gpt_batch_predict(0, X.p, Y.p, in.n_begin.p, 3, 3, 3, in.ls.p, 3, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_MATERN52, Xq.p, q_begin.p, nullptr,
                           nullptr, mean.p, nullptr, nullptr, status.p), GPT_E_ARG);
    CHECK(lml.all(SENT) && grad.all(SENT) && alpha.all(SENT) && mean.all(SENT) && status.all(ISENT));
}

// ---- batch search -------------------------------------------------------------------------------------------------------------
// R runs spread over the models (run r: model r % B), ending after 1 .. slices launches (stub_opt_launches): the relaunch loop
// makes exactly `slices` rounds, one launch per size class that still has a live run, and compacts its list between them.  A
// run that has ended holds zeros in its outputs and its number of launches in `evaluations`; the runs of the failed model end at
// once as GPT_OPT_NOT_PD_START with their clipped start still in theta.
void batch_opt_cases(const BatchShape& s, int64_t R, int slices, int failed) {
    const int64_t B = s.B();
    BatchInputs in(s);
    const size_t rows = (size_t)in.n_begin.p[B], P = 2 + (size_t)s.n_ls;
    D X = ramp(rows * s.Dm), Y = ramp(rows * s.O), theta0 = ramp(R * P, -3.0, 0.5), bounds(2 * P, 0.0);
    for (size_t i = 0; i < P; ++i) { bounds.p[2 * i] = i == 0 ? 1.0 : -2.0; bounds.p[2 * i + 1] = i == 0 ? 1.0 : 2.0; }   // c fixed
    Arr<int> run_model(R, 0);
    for (int64_t r = 0; r < R; ++r) run_model.p[r] = (int)(r % B);
    begin("gpt_batch_optimize " + s.name() + " R=" + std::to_string(R) + " slices=" + std::to_string(slices) +
          (failed >= 0 ? " failed=" + std::to_string(failed) : ""));
    gpt::stub_fail_model = failed;
    gpt::stub_opt_launches = slices;
    gpt::stub_opt_launch_count = 0;
    D theta(R * P, SENT), lml(R, SENT);
    Arr<int> iters(R, ISENT), evals(R, ISENT), status(R, ISENT);
    done(gpt_batch_optimize(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, s.n_ls, run_model.p, theta0.p, R, bounds.p, 1e-10, GPT_KERNEL_MATERN52,
                            1e-5, 2.22e-9, 15000, 15000, 7, theta.p, lml.p, iters.p, evals.p, status.p), GPT_OK);
    int want_launches = 0;
    for (int cls = 0; cls < 2; ++cls) {
        int longest = 0;
        for (int64_t r = 0; r < R; ++r)
            if ((s.n[r % B] > 32) == (cls == 1)) longest = std::max(longest, r % B == failed ? 1 : 1 + (int)(r % slices));
        want_launches += longest;
    }
    CHECK(gpt::stub_opt_launch_count == want_launches);
    for (int64_t r = 0; r < R; ++r) {
        const bool not_pd = r % B == failed;
        CHECK(status.p[r] == (not_pd ? GPT_OPT_NOT_PD_START : GPT_OPT_PGTOL));
        CHECK(evals.p[r] == (not_pd ? 1 : 1 + (int)(r % slices)) && iters.p[r] == 0 && lml.p[r] == 0.0);
        for (size_t i = 0; i < P; ++i) {
            const double clipped = std::min(std::max(theta0.p[r * P + i], bounds.p[2 * i]), bounds.p[2 * i + 1]);
            CHECK(theta.p[r * P + i] == (not_pd ? clipped : 0.0));
        }
    }
    gpt::stub_fail_model = -1;
    gpt::stub_opt_launches = 1;
}

void batch_opt_refusals() {
    BatchShape s{{1, 32, 33}, 3, 3, 3};
    BatchInputs in(s);
    D X = ramp(66 * 3), Y = ramp(66 * 3), theta0 = ramp(4 * 5, -1.0, 0.1), theta(4 * 5, SENT), lml(4, SENT);
    D bounds{-2, 2, -2, 2, -2, 2, -2, 2, -2, 2};
    Arr<int> run_model{0, 1, 2, 2}, iters(4, ISENT), evals(4, ISENT), status(4, ISENT);
    auto call = [&](const int* rm, int64_t R, const double* bd, const double* t0, double pgtol, int max_evals, int per_launch) {
        return gpt_batch_optimize(0, X.p, Y.p, in.n_begin.p, 3, 3, 3, 3, rm, t0, R, bd, 1e-10, GPT_KERNEL_RBF, pgtol, 2.22e-9, 15000, max_evals,
                                  per_launch, theta.p, lml.p, iters.p, evals.p, status.p);
    };
    begin("gpt_batch_optimize refuses R = 0"); done(call(run_model.p, 0, bounds.p, theta0.p, 1e-5, 15000, 64), GPT_E_ARG);
    begin("gpt_batch_optimize refuses run_model = NULL"); done(call(nullptr, 4, bounds.p, theta0.p, 1e-5, 15000, 64), GPT_E_ARG);
    Arr<int> outside{0, 1, 3, 2};
    begin("gpt_batch_optimize refuses run_model = B"); done(call(outside.p, 4, bounds.p, theta0.p, 1e-5, 15000, 64), GPT_E_ARG);
    D crossed{-2, 2, 2, -2, -2, 2, -2, 2, -2, 2};
    begin("gpt_batch_optimize refuses lo > hi"); done(call(run_model.p, 4, crossed.p, theta0.p, 1e-5, 15000, 64), GPT_E_ARG);
    D nan0(theta0);
    nan0.p[7] = std::nan("");
    begin("gpt_batch_optimize refuses NaN in theta0"); done(call(run_model.p, 4, bounds.p, nan0.p, 1e-5, 15000, 64), GPT_E_ARG);
    begin("gpt_batch_optimize refuses pgtol = 0"); done(call(run_model.p, 4, bounds.p, theta0.p, 0.0, 15000, 64), GPT_E_ARG);
    begin("gpt_batch_optimize refuses max_evals = 0"); done(call(run_model.p, 4, bounds.p, theta0.p, 1e-5, 0, 64), GPT_E_ARG);
    begin("gpt_batch_optimize refuses evals_per_launch = 0"); done(call(run_model.p, 4, bounds.p, theta0.p, 1e-5, 15000, 0), GPT_E_ARG);
    CHECK(theta.all(SENT) && lml.all(SENT) && iters.all(ISENT) && evals.all(ISENT) && status.all(ISENT));
}

// gpt_batch_optimize_bounded: a box per run (the boxes differ from run to run, some with a fixed component); the start of every run
// is clipped to its own box, which a run of the failed model shows in theta.
void batch_opt_bounded_cases(const BatchShape& s, int64_t R, int slices, int failed) {
    const int64_t B = s.B();
    BatchInputs in(s);
    const size_t rows = (size_t)in.n_begin.p[B], P = 2 + (size_t)s.n_ls;
    D X = ramp(rows * s.Dm), Y = ramp(rows * s.O), theta0 = ramp(R * P, -3.0, 0.5), bounds(R * 2 * P, 0.0);
    for (int64_t r = 0; r < R; ++r)
        for (size_t i = 0; i < P; ++i) {
            bounds.p[(r * P + i) * 2] = i == 0 && r % 2 ? 1.0 : -2.0 + 0.25 * (double)(r % 5);
            bounds.p[(r * P + i) * 2 + 1] = i == 0 && r % 2 ? 1.0 : 2.0 + 0.5 * (double)(r % 3);
        }
    Arr<int> run_model(R, 0);
    for (int64_t r = 0; r < R; ++r) run_model.p[r] = (int)(r % B);
    begin("gpt_batch_optimize_bounded " + s.name() + " R=" + std::to_string(R) + " slices=" + std::to_string(slices) +
          (failed >= 0 ? " failed=" + std::to_string(failed) : ""));
    gpt::stub_fail_model = failed;
    gpt::stub_opt_launches = slices;
    D theta(R * P, SENT), lml(R, SENT);
    Arr<int> iters(R, ISENT), evals(R, ISENT), status(R, ISENT);
    done(gpt_batch_optimize_bounded(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, s.n_ls, run_model.p, theta0.p, R, bounds.p, 1e-10, GPT_KERNEL_RBF,
                                    1e-5, 2.22e-9, 15000, 15000, 7, theta.p, lml.p, iters.p, evals.p, status.p), GPT_OK);
    for (int64_t r = 0; r < R; ++r) {
        const bool not_pd = r % B == failed;
        CHECK(status.p[r] == (not_pd ? GPT_OPT_NOT_PD_START : GPT_OPT_PGTOL));
        CHECK(evals.p[r] == (not_pd ? 1 : 1 + (int)(r % slices)) && iters.p[r] == 0 && lml.p[r] == 0.0);
        for (size_t i = 0; i < P; ++i) {
            const double clipped = std::min(std::max(theta0.p[r * P + i], bounds.p[(r * P + i) * 2]), bounds.p[(r * P + i) * 2 + 1]);
            CHECK(theta.p[r * P + i] == (not_pd ? clipped : 0.0));
        }
    }
    gpt::stub_fail_model = -1;
    gpt::stub_opt_launches = 1;
    if (R < 2) return;
    D crossed(bounds);
    std::swap(crossed.p[((R - 1) * P + 1) * 2], crossed.p[((R - 1) * P + 1) * 2 + 1]);
    D theta2(R * P, SENT);
    begin("gpt_batch_optimize_bounded refuses lo > hi in the last run's box");
    done(gpt_batch_optimize_bounded(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, s.n_ls, run_model.p, theta0.p, R, crossed.p, 1e-10, GPT_KERNEL_RBF,
                                    1e-5, 2.22e-9, 15000, 15000, 7, theta2.p, lml.p, iters.p, evals.p, status.p), GPT_E_ARG);
    crossed.p[((R - 1) * P + 1) * 2] = std::nan("");
    begin("gpt_batch_optimize_bounded refuses NaN in the last run's box");
    done(gpt_batch_optimize_bounded(0, X.p, Y.p, in.n_begin.p, B, s.Dm, s.O, s.n_ls, run_model.p, theta0.p, R, crossed.p, 1e-10, GPT_KERNEL_RBF,
                                    1e-5, 2.22e-9, 15000, 15000, 7, theta2.p, lml.p, iters.p, evals.p, status.p), GPT_E_ARG);
    CHECK(theta2.all(SENT));
}

// ---- fold scan ----------------------------------------------------------------------------------------------------------------
// queries: M per member (ragged), or one entry {M} for queries that all members share (q_begin = NULL).  mask: bit 0 det, 1 z,
// 2 err.  A member that ran holds zeros in what was asked of it; the failed member keeps every sentinel, the member whose
// surrogate alone failed keeps those of err, err_sum and err_max, and without the surrogate nobody's err outputs are touched.
void fold_scan_cases(const BatchShape& s, const std::vector<int>& queries, bool shared, int surrogate, int failed, int failed_surrogate) {
    const int64_t B = s.B();
    BatchInputs in(s);
    const size_t rows = (size_t)in.n_begin.p[B];
    D X = ramp(rows * s.Dm), Y = ramp(rows * s.Dm);
    Arr<int64_t> o_begin(B + 1, 0), one_each(B + 1, 0);
    for (int64_t b = 0; b < B; ++b) { o_begin.p[b + 1] = o_begin.p[b] + (shared ? queries[0] : queries[b]); one_each.p[b + 1] = b + 1; }
    const size_t Mo = (size_t)o_begin.p[B], Mq = shared ? (size_t)queries[0] : Mo;
    D Xq = ramp(Mq * s.Dm);
    gpt::stub_fail_model = failed;
    gpt::stub_fail_surrogate = failed_surrogate;
    for (int mask : {0, 7, 1, 2, 4}) {
        begin("gpt_batch_fold_scan " + s.name() + (shared ? " shared" : " ragged") + " M=" + std::to_string(Mq) + " surrogate=" +
              std::to_string(surrogate) + " outputs=" + std::to_string(mask) + (failed >= 0 ? " failed=" + std::to_string(failed) : "") +
              (failed_surrogate >= 0 ? " failed_surrogate=" + std::to_string(failed_surrogate) : ""));
        D min_det(B, SENT), err_sum(B, SENT), err_max(B, SENT), det(Mo, SENT), z(Mo * s.Dm, SENT), err(Mo, SENT);
        Arr<int64_t> argmin(B, (int64_t)ISENT), n_fold(B, (int64_t)ISENT);
        Arr<int> status(B, ISENT), sur_status(B, ISENT);
        const bool with_null = !surrogate && (mask & 1);                 // without the surrogate its outputs may be NULL
        done(gpt_batch_fold_scan(0, X.p, Y.p, in.n_begin.p, B, s.Dm, in.ls.p, s.n_ls, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF,
                                 Mq ? Xq.p : nullptr, shared ? nullptr : o_begin.p, shared ? queries[0] : -1, surrogate, min_det.p, argmin.p,
                                 n_fold.p, with_null ? nullptr : err_sum.p, with_null ? nullptr : err_max.p, mask & 1 ? det.p : nullptr,
                                 mask & 2 ? z.p : nullptr, mask & 4 ? err.p : nullptr, status.p, with_null ? nullptr : sur_status.p), GPT_OK);
        check_status(status, failed);
        check_slices(min_det, one_each, 1, failed);
        for (int64_t b = 0; b < B; ++b) {
            const bool ran = b != failed, sur_ran = ran && surrogate && b != failed_surrogate;
            CHECK(argmin.p[b] == (ran ? 0 : (int64_t)ISENT) && n_fold.p[b] == (ran ? 0 : (int64_t)ISENT));
            CHECK(sur_status.p[b] == (!ran || !surrogate ? ISENT : (b == failed_surrogate ? GPT_E_NOT_PD : GPT_OK)));
            CHECK(err_sum.p[b] == (sur_ran ? 0.0 : SENT) && err_max.p[b] == (sur_ran ? 0.0 : SENT));
            CHECK(err.all(sur_ran && (mask & 4) ? 0.0 : SENT, (size_t)o_begin.p[b], (size_t)o_begin.p[b + 1]));
        }
        if (mask & 1) check_slices(det, o_begin, 1, failed);
        else CHECK(det.all(SENT));
        if (mask & 2) check_slices(z, o_begin, s.Dm, failed);
        else CHECK(z.all(SENT));
    }
    gpt::stub_fail_model = -1;
    gpt::stub_fail_surrogate = -1;
}

void fold_scan_refusals() {
    BatchShape s{{1, 32, 33}, 3, 3, 3};
    BatchInputs in(s);
    D X = ramp(66 * 4), Y = ramp(66 * 4), Xq = ramp(5 * 3), out(3, SENT);
    Arr<int64_t> iout(3, (int64_t)ISENT), q_begin{0, 1, 3, 5};
    Arr<int> status(3, ISENT);
    auto call = [&](const int64_t* nb, int64_t B, int Dm, int ktype, const double* xq, const int64_t* qb, int64_t M, int surrogate, double* es) {
        return gpt_batch_fold_scan(0, X.p, Y.p, nb, B, Dm, in.ls.p, Dm, in.c.p, in.noise.p, 1e-10, ktype, xq, qb, M, surrogate, out.p, iout.p, iout.p,
                                   es, es, nullptr, nullptr, nullptr, status.p, status.p);
    };
    begin("gpt_batch_fold_scan refuses D = 4"); done(call(in.n_begin.p, 3, 4, GPT_KERNEL_RBF, Xq.p, q_begin.p, 0, 0, nullptr), GPT_E_ARG);
    begin("gpt_batch_fold_scan refuses a Matern batch"); done(call(in.n_begin.p, 3, 3, GPT_KERNEL_MATERN32, Xq.p, q_begin.p, 0, 0, nullptr), GPT_E_ARG);
    Arr<int64_t> too_many{0, 129};
    D X129 = ramp(129 * 3);
    begin("gpt_batch_fold_scan refuses n_b = 129");
    done(gpt_batch_fold_scan(0, X129.p, X129.p, too_many.p, 1, 3, in.ls.p, 3, in.c.p, in.noise.p, 1e-10, GPT_KERNEL_RBF, Xq.p, nullptr, 5, 0, out.p,
                             iout.p, iout.p, nullptr, nullptr, nullptr, nullptr, nullptr, status.p, nullptr), GPT_E_ARG);
    Arr<int64_t> falling{0, 3, 2, 5};
    begin("gpt_batch_fold_scan refuses a falling q_begin"); done(call(in.n_begin.p, 3, 3, GPT_KERNEL_RBF, Xq.p, falling.p, 0, 0, nullptr), GPT_E_ARG);
    D nanq(Xq);
    nanq.p[14] = std::nan("");
    begin("gpt_batch_fold_scan refuses NaN in Xq (ragged)"); done(call(in.n_begin.p, 3, 3, GPT_KERNEL_RBF, nanq.p, q_begin.p, 0, 0, nullptr), GPT_E_ARG);
    begin("gpt_batch_fold_scan refuses NaN in Xq (shared)"); done(call(in.n_begin.p, 3, 3, GPT_KERNEL_RBF, nanq.p, nullptr, 5, 0, nullptr), GPT_E_ARG);
    begin("gpt_batch_fold_scan refuses M < 0"); done(call(in.n_begin.p, 3, 3, GPT_KERNEL_RBF, Xq.p, nullptr, -1, 0, nullptr), GPT_E_ARG);
    begin("gpt_batch_fold_scan refuses err_sum = NULL with the surrogate");
    done(call(in.n_begin.p, 3, 3, GPT_KERNEL_RBF, Xq.p, q_begin.p, 0, 1, nullptr), GPT_E_ARG);
    CHECK(out.all(SENT) && iout.all((int64_t)ISENT) && status.all(ISENT));
}

// ---- select -------------------------------------------------------------------------------------------------------------------
void select_cases() {
    const int64_t N = 5;
    for (int Dm : {1, 3, 4, 9})
        for (int n_total : {1, 4, 5})
            for (int n_initial : {0, 2, n_total})
                for (int with_residual = 0; with_residual < 2; ++with_residual)
                    for (int failing = 0; failing < 2; ++failing) {
                        if (n_initial > n_total || (failing && (with_residual || n_initial == 2))) continue;
                        begin("gpt_select_greedy D=" + std::to_string(Dm) + " n_total=" + std::to_string(n_total) + " n_initial=" +
                              std::to_string(n_initial) + (with_residual ? " residual" : "") + (failing ? " failure flag" : ""));
                        D X = ramp(N * Dm), ls = ramp(Dm, 0.5), selvar(n_total - n_initial, SENT), residual(N, SENT);
                        Arr<int64_t> initial(n_initial, 0), selected(n_total, ISENT);
                        for (int t = 0; t < n_initial; ++t) initial.p[t] = N - 1 - t;
                        gpt::stub_fail_flag = failing;
                        done(gpt_select_greedy(0, X.p, N, Dm, ls.p, 1.0, 0.01, 1e-10, GPT_KERNEL_MATERN52, n_initial ? initial.p : nullptr, n_initial,
                                               n_total, selected.p, n_initial == n_total ? nullptr : selvar.p, with_residual ? residual.p : nullptr),
                             failing ? GPT_E_NOT_PD : GPT_OK);
                        gpt::stub_fail_flag = false;
                        if (failing) { CHECK(selected.all(ISENT) && selvar.all(SENT) && residual.all(SENT)); continue; }
                        std::vector<int> seen(N, 0);
                        for (int t = 0; t < n_total; ++t) {
                            CHECK(selected.p[t] >= 0 && selected.p[t] < N && !seen[selected.p[t]]++);
                            if (t < n_initial) CHECK(selected.p[t] == initial.p[t]);
                        }
                        CHECK(std::none_of(selvar.p, selvar.p + selvar.n, [](double v) { return v == SENT; }));
                        CHECK(with_residual ? std::none_of(residual.p, residual.p + N, [](double v) { return v == SENT; }) : residual.all(SENT));
                    }
    D X = ramp(N * 3), ls = ramp(3, 0.5), selvar(5, SENT);
    Arr<int64_t> selected(5, ISENT), bad_initial{1, 5}, twice{2, 2};
    auto select = [&](const double* x, int Dm, const int64_t* initial, int n_initial, int n_total) {
        return gpt_select_greedy(0, x, N, Dm, ls.p, 1.0, 0.01, 1e-10, GPT_KERNEL_RBF, initial, n_initial, n_total, selected.p, selvar.p, nullptr);
    };
    begin("gpt_select_greedy refuses X = NULL"); done(select(nullptr, 3, nullptr, 0, 2), GPT_E_ARG);
    begin("gpt_select_greedy refuses D = 16"); done(select(X.p, 16, nullptr, 0, 2), GPT_E_ARG);
    begin("gpt_select_greedy refuses n_total > N"); done(select(X.p, 3, nullptr, 0, 6), GPT_E_ARG);
    begin("gpt_select_greedy refuses an initial index out of range"); done(select(X.p, 3, bad_initial.p, 2, 3), GPT_E_ARG);
    begin("gpt_select_greedy refuses an initial index listed twice"); done(select(X.p, 3, twice.p, 2, 3), GPT_E_ARG);
    CHECK(selected.all(ISENT) && selvar.all(SENT));
}

// ---- SVGP trainers ------------------------------------------------------------------------------------------------------------
using TrainFn = int (*)(int, const double*, const double*, int64_t, int, int, int, double*, double*, double*, double*, double*, double*,
                        const int64_t*, int64_t, const int64_t*, int64_t, double, double*);
using GradFn = int (*)(int, const double*, const double*, int64_t, int64_t, int, int, int, const double*, const double*, const double*,
                       const double*, const double*, const double*, double*, double*, double*, double*, double*, double*, double*);

struct SvgpParams {
    D Z, m, C, raw_ls, raw_os, raw_noise;
    SvgpParams(int T, int Zn, int Dm, size_t n_ls, double fill)
        : Z(Zn * Dm, fill), m(T * Zn, fill), C((size_t)T * Zn * Zn, fill), raw_ls(n_ls, fill), raw_os(T, fill), raw_noise(T + 1, fill) {}
    D& at(int q) { D* a[6] = {&Z, &m, &C, &raw_ls, &raw_os, &raw_noise}; return *a[q]; }
};
constexpr double UPPER = 77.0;       // the strict upper triangle of C: not a parameter, returned as passed

SvgpParams svgp_params(int T, int Zn, int Dm, size_t n_ls) {
    SvgpParams p(T, Zn, Dm, n_ls, 0.0);
    for (int q = 0; q < 6; ++q)
        for (size_t i = 0; i < p.at(q).n; ++i) p.at(q).p[i] = 0.25 + 0.125 * (double)(i % 13);
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < Zn; ++i)
            for (int j = i + 1; j < Zn; ++j) p.C.p[((size_t)t * Zn + i) * Zn + j] = UPPER;
    return p;
}

void svgp_cases(const std::string& unit, TrainFn train, GradFn elbo_grad, bool ls_per_task) {
    const int64_t N = 7;
    for (auto [T, Zn, Dm] : {std::array<int, 3>{1, 1, 1}, std::array<int, 3>{3, 5, 2}}) {
        const size_t n_ls = ls_per_task ? (size_t)T * Dm : (size_t)Dm;
        const std::string shape = " T=" + std::to_string(T) + " Z=" + std::to_string(Zn) + " D=" + std::to_string(Dm);
        D X = ramp(N * Dm), Y = ramp(N * T);
        // the schedule starts past idx[0], which is no row of X (an upload that is not offset by batch_begin[0] hands it to the
        // stand-in kernels, which refuse it); batches of 3, 1 and 2 rows
        Arr<int64_t> idx{99, 0, 3, 5, 2, 6, 1}, bb{1, 4, 5, 7};
        for (int failing = 0; failing < 2; ++failing) {
            begin(unit + "_train" + shape + (failing ? " failure flag" : ""));
            SvgpParams p = svgp_params(T, Zn, Dm, n_ls);
            SvgpParams passed = svgp_params(T, Zn, Dm, n_ls);
            D loss(3, SENT);
            gpt::stub_fail_flag = failing;
            done(train(0, X.p, Y.p, N, Dm, T, Zn, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, p.raw_noise.p, idx.p, (int64_t)idx.n, bb.p, 3, 0.01,
                       loss.p), failing ? GPT_E_NOT_PD : GPT_OK);
            gpt::stub_fail_flag = false;
            if (failing) {
                for (int q = 0; q < 6; ++q) CHECK(p.at(q).same(passed.at(q)));
                CHECK(loss.all(SENT));
                continue;
            }
            CHECK(loss.all(0.0) && p.Z.all(0.0) && p.m.all(0.0) && p.raw_ls.all(0.0) && p.raw_os.all(0.0) && p.raw_noise.all(0.0));
            for (int t = 0; t < T; ++t)
                for (int i = 0; i < Zn; ++i)
                    for (int j = 0; j < Zn; ++j) CHECK(p.C.p[((size_t)t * Zn + i) * Zn + j] == (j <= i ? 0.0 : UPPER));
        }
        for (int mask : {63, 21, 42}) {                                  // all gradients; every second one NULL, either way round
            begin(unit + "_elbo_grad" + shape + " gradients=" + std::to_string(mask));
            SvgpParams p = svgp_params(T, Zn, Dm, n_ls), g(T, Zn, Dm, n_ls, SENT);
            D loss(1, SENT), Xb = ramp(3 * Dm), Yb = ramp(3 * T);
            double* gp[6];
            for (int q = 0; q < 6; ++q) gp[q] = (mask >> q & 1) ? g.at(q).p : nullptr;
            done(elbo_grad(0, Xb.p, Yb.p, 3, N, Dm, T, Zn, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, p.raw_noise.p, loss.p, gp[0], gp[1], gp[2],
                           gp[3], gp[4], gp[5]), GPT_OK);
            CHECK(loss.all(0.0));
            for (int q = 0; q < 6; ++q) CHECK(g.at(q).all(gp[q] ? 0.0 : SENT));
        }
    }
    D X = ramp(N * 2), Y = ramp(N * 3), loss(1, SENT);
    SvgpParams p = svgp_params(3, 5, 2, ls_per_task ? 6 : 2);
    Arr<int64_t> idx{0, 1, 7}, bb{0, 3};
    auto run = [&](const double* x, int Dm, int64_t last) {
        return train(0, x, Y.p, N, Dm, 3, 5, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, p.raw_noise.p, idx.p, 3, bb.p, last, 0.01, loss.p);
    };
    begin(unit + "_train refuses X = NULL"); done(run(nullptr, 2, 1), GPT_E_ARG);
    begin(unit + "_train refuses D = 16"); done(run(X.p, 16, 1), GPT_E_ARG);
    begin(unit + "_train refuses an empty schedule"); done(run(X.p, 2, 0), GPT_E_ARG);
    begin(unit + "_train refuses a schedule index out of range"); done(run(X.p, 2, 1), GPT_E_ARG);
    begin(unit + "_elbo_grad refuses b = 0");
    done(elbo_grad(0, X.p, Y.p, 0, N, 2, 3, 5, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, p.raw_noise.p, loss.p, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr), GPT_E_ARG);
    CHECK(loss.all(SENT));
}

void surface_predict_cases() {
    for (auto [T, Zn, Dm] : {std::array<int, 3>{1, 1, 1}, std::array<int, 3>{3, 5, 2}}) {
        const SvgpParams p = svgp_params(T, Zn, Dm, (size_t)T * Dm);
        for (int64_t M : {(int64_t)1, (int64_t)64, (int64_t)65, (int64_t)1025})      // 1025: one query past a whole prediction chunk
            for (int mask : {0, 3, 1, 2})
                for (int failing = 0; failing < 2; ++failing) {
                    if (failing && (mask != 3 || M != 65)) continue;
                    begin("gpt_svgp_surface_predict T=" + std::to_string(T) + " Z=" + std::to_string(Zn) + " D=" + std::to_string(Dm) + " M=" +
                          std::to_string(M) + (mask & 1 ? " var" : "") + (mask & 2 ? " J" : "") + (failing ? " failure flag" : ""));
                    D Xq = ramp(M * Dm), mean(M * T, SENT), var(M * T, SENT), J((size_t)M * T * Dm, SENT);
                    gpt::stub_fail_flag = failing;
                    done(gpt_svgp_surface_predict(0, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, Zn, Dm, T, Xq.p, M, mean.p, mask & 1 ? var.p : nullptr,
                                                  mask & 2 ? J.p : nullptr), failing ? GPT_E_NOT_PD : GPT_OK);
                    gpt::stub_fail_flag = false;
                    CHECK(mean.all(failing ? SENT : 0.0));
                    CHECK(var.all(!failing && (mask & 1) ? 0.0 : SENT) && J.all(!failing && (mask & 2) ? 0.0 : SENT));
                }
    }
    const SvgpParams p = svgp_params(3, 5, 2, 6);
    D Xq = ramp(2), mean(3, SENT);
    auto predict = [&](const double* xq, int Dm, int64_t M) {
        return gpt_svgp_surface_predict(0, p.Z.p, p.m.p, p.C.p, p.raw_ls.p, p.raw_os.p, 5, Dm, 3, xq, M, mean.p, nullptr, nullptr);
    };
    begin("gpt_svgp_surface_predict refuses Xq = NULL"); done(predict(nullptr, 2, 1), GPT_E_ARG);
    begin("gpt_svgp_surface_predict refuses D = 16"); done(predict(Xq.p, 16, 1), GPT_E_ARG);
    begin("gpt_svgp_surface_predict refuses M = 0"); done(predict(Xq.p, 2, 0), GPT_E_ARG);
    CHECK(mean.all(SENT));
}

// ---- inverse map (gpt_api.hip): one image carved into Y | Z0 | Z | residual | det | passes | status ----------------------------
void inverse_map_cases() {
    const int64_t N = 5;
    D X = ramp(N * 2), Y = ramp(N * 2, 0.01, 0.01), ls{0.5, 0.75};
    gpt_handle* h = nullptr;
    begin("gpt_inverse_map setup");
    CHECK(gpt_create(&h, 0) == GPT_OK);
    // the handle keeps its own buffers, so a case ends with as many live objects as `held`, not with none
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    D Y1 = ramp(2), Z1(2, SENT);
    Arr<int> status1(1, ISENT);
    auto refused = [&](gpt_handle* hh, const double* y, int64_t M, double rtol, int max_passes, double* z) {
        return gpt_inverse_map(hh, y, nullptr, M, rtol, max_passes, z, nullptr, nullptr, nullptr, status1.p);
    };
    begin("gpt_inverse_map refuses a handle without a model"); done_held(refused(h, Y1.p, 1, 1e-10, 50, Z1.p), GPT_E_STATE);
    CHECK(gpt_fit(h, X.p, Y.p, N, 2, 2, ls.p, 2, 1.0, 0.01, 1e-10) == GPT_OK);
    held = stub_live_objects;
    begin("gpt_inverse_map refuses a NULL handle"); done_held(refused(nullptr, Y1.p, 1, 1e-10, 50, Z1.p), GPT_E_ARG);
    begin("gpt_inverse_map refuses Y = NULL"); done_held(refused(h, nullptr, 1, 1e-10, 50, Z1.p), GPT_E_ARG);
    begin("gpt_inverse_map refuses Z = NULL"); done_held(refused(h, Y1.p, 1, 1e-10, 50, nullptr), GPT_E_ARG);
    begin("gpt_inverse_map refuses M = -1"); done_held(refused(h, Y1.p, -1, 1e-10, 50, Z1.p), GPT_E_ARG);
    begin("gpt_inverse_map refuses rtol = 0"); done_held(refused(h, Y1.p, 1, 0.0, 50, Z1.p), GPT_E_ARG);
    begin("gpt_inverse_map refuses max_passes = 0"); done_held(refused(h, Y1.p, 1, 1e-10, 0, Z1.p), GPT_E_ARG);
    CHECK(Z1.all(SENT) && status1.all(ISENT));
    for (int64_t M : {(int64_t)1, (int64_t)3})                          // growing: each call gets an image of its exact size
        for (int mask : {0, 15, 5, 10}) {
            begin("gpt_inverse_map M=" + std::to_string(M) + " optional=" + std::to_string(mask));
            D Yt = ramp(M * 2), Z0 = ramp(M * 2), Z(M * 2, SENT), residual(M, SENT), det(M, SENT);
            Arr<int> passes(M, ISENT), status(M, ISENT);
            const int rc = gpt_inverse_map(h, Yt.p, mask & 1 ? Z0.p : nullptr, M, 1e-10, 50, Z.p, mask & 2 ? residual.p : nullptr,
                                           mask & 4 ? det.p : nullptr, mask & 8 ? passes.p : nullptr, status.p);
            if (M == 1 && mask == 0) { CHECK(stub_live_objects == held + 1); held = stub_live_objects; }   // the one image, kept and regrown
            done_held(rc, GPT_OK);
            CHECK(Z.all(0.0) && status.all(0) && residual.all(mask & 2 ? 0.0 : SENT) && det.all(mask & 4 ? 0.0 : SENT));
            CHECK(passes.all(mask & 8 ? 0 : ISENT));
        }
    begin("gpt_inverse_map teardown");
    gpt_destroy(h);
    done(GPT_OK, GPT_OK);
}

// ---- predict_all (gpt_api.hip): chunks of HOST_CHUNK through the handle's two staging sets in the model's element type T; dvar is
// (D, M) plane-major, a chunk's image (D, m) ----------------------------------------------------------------------------------------
template <class T> void predict_all_cases(int dtype, const char* tname) {
    const int64_t N = 5, HOST_CHUNK = 1 << 17;
    const T sent = (T)-7.25e30;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), ls{0.5, 0.75, 0.6};
    const std::string who = std::string("gpt_predict_all ") + tname;
    gpt_handle* h = nullptr;
    begin(who + " setup");
    CHECK(gpt_create(&h, 0) == GPT_OK && gpt_set_dtype(h, dtype) == GPT_OK);
    CHECK(gpt_fit(h, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    long held = stub_live_objects;
    enum { MEAN, VAR, J, JVAR, DVAR, N_OUT };                // bit k of `mask`: output k is asked for
    const size_t width[N_OUT] = {3, 1, 9, 3, 3};
    std::vector<int> masks;
    const int ALL = (1 << N_OUT) - 1;
    for (int k = 0; k < N_OUT; ++k) { masks.push_back(1 << k); masks.push_back(ALL & ~(1 << k)); }
    for (int64_t M : {(int64_t)0, (int64_t)1, (int64_t)3, HOST_CHUNK - 1, HOST_CHUNK, HOST_CHUNK + 1, 2 * HOST_CHUNK + 3})   // growing; the last three walk both staging sets
        for (int mask : masks) {
            begin(who + " M=" + std::to_string(M) + " outputs=" + std::to_string(mask));
            Arr<T> Xq((size_t)M * 3, (T)0.5);
            std::vector<Arr<T>> out;
            for (int k = 0; k < N_OUT; ++k) out.emplace_back((size_t)M * width[k], sent);
            T* p[N_OUT];
            for (int k = 0; k < N_OUT; ++k) p[k] = (mask >> k & 1) ? out[k].p : nullptr;
            const int rc = gpt_predict_all(h, Xq.p, M, p[MEAN], p[VAR], p[J], p[JVAR], p[DVAR]);
            CHECK(rc == GPT_OK);
            CHECK(stub_live_objects >= held);                            // staging and the variance workspace are kept and regrown, never dropped
            held = stub_live_objects;
            for (int k = 0; k < N_OUT; ++k) CHECK(out[k].all(mask >> k & 1 ? (T)0 : sent));
            printf("ok  %s\n", g_case.c_str());
            ++g_cases;
        }
    begin(who + " teardown");
    gpt_destroy(h);
    done(GPT_OK, GPT_OK);
}

// ---- transport (gpt_transport_host.hip): chunks of HOST_CHUNK through two staging sets, one buffer per array asked for ----------
void transport_cases() {
    const int64_t N = 5, HOST_CHUNK = 1 << 17;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle* h = nullptr;
    begin("gpt_transport_policy setup");
    CHECK(gpt_create(&h, 0) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    // bit k of `mask`: optional array k is passed
    enum { VEL, ORI, POS_ROT, VAR, VEL_OUT, VEL_VAR, DET_VEL, ORI_OUT, DET_ORI, ORI_GAP, POST_MEAN, POST_J, POST_JVAR, POST_J_ORI, N_OPT };
    const size_t width[N_OPT] = {3, 4, 3, 1, 3, 1, 1, 4, 1, 1, 3, 9, 3, 9};
    struct Arrays {
        D pos, pos_out;
        std::vector<D> opt;
        Arrays(int64_t M, const size_t* w) : pos(ramp(M * 3)), pos_out(M * 3, SENT) {
            for (int k = 0; k < N_OPT; ++k) opt.push_back(k < 2 ? ramp(M * w[k]) : D(M * w[k], SENT));
        }
    };
    auto call = [&](gpt_handle* hh, Arrays& a, int64_t M, int mask, const double* pos, double* pos_out) {
        double* p[N_OPT];
        for (int k = 0; k < N_OPT; ++k) p[k] = (mask >> k & 1) ? a.opt[k].p : nullptr;
        return gpt_transport_policy(hh, pos, M, R.p, c_src.p, c_dst.p, 1.25, R.p, p[VEL], p[ORI], p[POS_ROT], pos_out, p[VAR], p[VEL_OUT],
                                    p[VEL_VAR], p[DET_VEL], p[ORI_OUT], p[DET_ORI], p[ORI_GAP], p[POST_MEAN], p[POST_J], p[POST_JVAR],
                                    p[POST_J_ORI]);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.pos_out.all(SENT));
        for (int k = 2; k < N_OPT; ++k) CHECK(a.opt[k].all(SENT));
    };
    const int ALL = (1 << N_OPT) - 1;
    {
        Arrays a(1, width);
        begin("gpt_transport_policy refuses a handle without a model"); done_held(call(h, a, 1, ALL, a.pos.p, a.pos_out.p), GPT_E_STATE);
        CHECK(gpt_fit(h, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        begin("gpt_transport_policy refuses a NULL handle"); done_held(call(nullptr, a, 1, ALL, a.pos.p, a.pos_out.p), GPT_E_ARG);
        begin("gpt_transport_policy refuses pos = NULL"); done_held(call(h, a, 1, ALL, nullptr, a.pos_out.p), GPT_E_ARG);
        begin("gpt_transport_policy refuses pos_out = NULL"); done_held(call(h, a, 1, ALL, a.pos.p, nullptr), GPT_E_ARG);
        begin("gpt_transport_policy refuses M = -1"); done_held(call(h, a, -1, ALL, a.pos.p, a.pos_out.p), GPT_E_ARG);
        begin("gpt_transport_policy refuses vel_out without vel"); done_held(call(h, a, 1, ALL & ~(1 << VEL), a.pos.p, a.pos_out.p), GPT_E_ARG);
        begin("gpt_transport_policy refuses ori_out without ori"); done_held(call(h, a, 1, ALL & ~(1 << ORI), a.pos.p, a.pos_out.p), GPT_E_ARG);
        D nan_pos{0.5, std::nan(""), 0.5};
        begin("gpt_transport_policy refuses NaN in pos"); done_held(call(h, a, 1, ALL, nan_pos.p, a.pos_out.p), GPT_E_ARG);
        begin("gpt_transport_policy M = 0 does nothing"); done_held(call(h, a, 0, ALL, a.pos.p, a.pos_out.p), GPT_OK);
        untouched(a);
    }
    // every optional array, none, and two complementary halves (an output never without its input)
    const int half_a = 1 << VEL | 1 << POS_ROT | 1 << VEL_OUT | 1 << DET_VEL | 1 << DET_ORI | 1 << POST_MEAN | 1 << POST_JVAR;
    const int half_b = 1 << ORI | 1 << VAR | 1 << ORI_OUT | 1 << ORI_GAP | 1 << POST_J | 1 << POST_J_ORI;
    const int var_alone = 1 << VEL | 1 << VEL_VAR;                       // the Jacobian variance without the variance
    for (int64_t M : {(int64_t)1, (int64_t)3, HOST_CHUNK + 1})           // growing; the last walks both staging sets
        for (int mask : {0, ALL, half_a, half_b, var_alone}) {
            if (M > 3 && mask != ALL) continue;
            begin("gpt_transport_policy M=" + std::to_string(M) + " optional=" + std::to_string(mask));
            Arrays a(M, width);
            const int rc = call(h, a, M, mask, a.pos.p, a.pos_out.p);
            CHECK(stub_live_objects >= held);                            // staging and scratch are kept and regrown, never dropped
            held = stub_live_objects;
            done_held(rc, GPT_OK);
            CHECK(a.pos_out.all(0.0));
            for (int k = 2; k < N_OPT; ++k) CHECK(a.opt[k].all(mask >> k & 1 ? 0.0 : SENT));
        }
    {
        begin("gpt_transport_policy refuses orientations of a 2-D model");
        D X2 = ramp(N * 2), Y2 = ramp(N * 2, 0.01, 0.01), ls2{0.5, 0.75};
        CHECK(gpt_fit(h, X2.p, Y2.p, N, 2, 2, ls2.p, 2, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        Arrays a(1, width);
        done_held(call(h, a, 1, 1 << ORI | 1 << DET_ORI, a.pos.p, a.pos_out.p), GPT_E_ARG);
        untouched(a);
    }
    begin("gpt_transport_policy teardown");
    gpt_destroy(h);
    done(GPT_OK, GPT_OK);
}

// ---- pull-back (gpt_transport_host.hip): two handles, chunks of HOST_CHUNK through the map handle's two staging sets, int and double arrays ---
void pullback_cases() {
    const int64_t N = 5, Nd = 7, HOST_CHUNK = 1 << 17;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h = nullptr, *hd = nullptr;
    begin("gpt_pullback_policy setup");
    CHECK(gpt_create(&h, 0) == GPT_OK && gpt_create(&hd, 0) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    // bit k of `mask`: optional array k is passed (X0 is the one optional input)
    enum { X0, XO, F, DET, RES, PASSES, VAR_DYN, MAP_VAR, VVAR_MAP, VVAR_DYN, POST_Z, POST_A, POST_JVAR, N_OPT };
    const size_t width[N_OPT] = {3, 3, 3, 1, 1, 0, 1, 1, 1, 3, 3, 9, 3};
    struct Arrays {
        D y, vel;
        Arr<int> status, passes;
        std::vector<D> opt;
        Arrays(int64_t M, const size_t* w) : y(ramp(M * 3)), vel(M * 3, SENT), status(M, ISENT), passes(M, ISENT) {
            for (int k = 0; k < N_OPT; ++k) opt.push_back(k == X0 ? ramp(M * w[k]) : D(M * w[k], SENT));
        }
    };
    auto call = [&](gpt_handle* hm, gpt_handle* hdyn, Arrays& a, int64_t M, int mask, const double* y, double* vel, int* status,
                    double rtol = 1e-10, int max_passes = 50) {
        double* p[N_OPT];
        for (int k = 0; k < N_OPT; ++k) p[k] = (mask >> k & 1) ? a.opt[k].p : nullptr;
        return gpt_pullback_policy(hm, hdyn, y, p[X0], M, R.p, c_src.p, c_dst.p, 1.25, R.p, rtol, max_passes, 0.1, p[XO], vel, p[F], p[DET],
                                   p[RES], (mask >> PASSES & 1) ? a.passes.p : nullptr, status, p[VAR_DYN], p[MAP_VAR], p[VVAR_MAP],
                                   p[VVAR_DYN], p[POST_Z], p[POST_A], p[POST_JVAR]);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.vel.all(SENT) && a.status.all(ISENT) && a.passes.all(ISENT));
        for (int k = 1; k < N_OPT; ++k) CHECK(a.opt[k].all(SENT));
    };
    const int ALL = (1 << N_OPT) - 1;
    {
        Arrays a(1, width);
        begin("gpt_pullback_policy refuses a map handle without a model"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_STATE);
        CHECK(gpt_fit(h, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        begin("gpt_pullback_policy refuses a dynamics handle without a model"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_STATE);
        CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        begin("gpt_pullback_policy refuses a NULL map handle"); done_held(call(nullptr, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses a NULL dynamics handle"); done_held(call(h, nullptr, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses one handle twice"); done_held(call(h, h, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses y = NULL"); done_held(call(h, hd, a, 1, ALL, nullptr, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses vel = NULL"); done_held(call(h, hd, a, 1, ALL, a.y.p, nullptr, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses status = NULL"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, nullptr), GPT_E_ARG);
        begin("gpt_pullback_policy refuses M = -1"); done_held(call(h, hd, a, -1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy refuses rtol = 0"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p, 0.0), GPT_E_ARG);
        begin("gpt_pullback_policy refuses rtol = NaN"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p, std::nan("")), GPT_E_ARG);
        begin("gpt_pullback_policy refuses max_passes = 0"); done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p, 1e-10, 0), GPT_E_ARG);
        D nan_y{0.5, std::nan(""), 0.5};
        begin("gpt_pullback_policy refuses NaN in y"); done_held(call(h, hd, a, 1, ALL, nan_y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_policy M = 0 does nothing"); done_held(call(h, hd, a, 0, ALL, a.y.p, a.vel.p, a.status.p), GPT_OK);
        untouched(a);
    }
    // every optional array on and off: none, all, each one alone, all but each one; then the staging arithmetic around HOST_CHUNK
    std::vector<int> masks{0, ALL};
    for (int k = 0; k < N_OPT; ++k) { masks.push_back(1 << k); masks.push_back(ALL & ~(1 << k)); }
    for (int64_t M : {(int64_t)1, (int64_t)3, HOST_CHUNK - 1, HOST_CHUNK, HOST_CHUNK + 1, 2 * HOST_CHUNK + 3})   // growing; the last three walk both staging sets
        for (int mask : masks) {
            if (M > 3 && mask != ALL && mask != 0) continue;
            begin("gpt_pullback_policy M=" + std::to_string(M) + " optional=" + std::to_string(mask));
            Arrays a(M, width);
            const int rc = call(h, hd, a, M, mask, a.y.p, a.vel.p, a.status.p);
            CHECK(stub_live_objects >= held);                            // staging, scratch and events are kept and regrown, never dropped
            held = stub_live_objects;
            done_held(rc, GPT_OK);
            CHECK(a.vel.all(0.0) && a.status.all(0) && a.passes.all(mask >> PASSES & 1 ? 0 : ISENT));
            for (int k = 1; k < N_OPT; ++k) CHECK(a.opt[k].all(mask >> k & 1 ? 0.0 : SENT));
        }
    {
        begin("gpt_pullback_policy refuses models of different dimension");
        D X2 = ramp(Nd * 2), Y2 = ramp(Nd * 2, 0.01, 0.01), ls2{0.5, 0.75};
        CHECK(gpt_fit(hd, X2.p, Y2.p, Nd, 2, 2, ls2.p, 2, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        Arrays a(1, width);
        done_held(call(h, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        untouched(a);
    }
    begin("gpt_pullback_policy teardown");
    gpt_destroy(h);
    gpt_destroy(hd);
    done(GPT_OK, GPT_OK);
}

// ---- chain of pull-backs (gpt_chain_host.hip): K + 1 handles, stage-major (K, M, ...) arrays through the last stage's two staging sets
void chain_cases() {
    const int64_t N = 5, Nd = 7, HOST_CHUNK = 1 << 17;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h[GPT_CHAIN_MAX + 1] = {}, *hd = nullptr, *bare = nullptr;
    begin("gpt_pullback_chain setup");
    for (auto& q : h) CHECK(gpt_create(&q, 0) == GPT_OK);
    CHECK(gpt_create(&hd, 0) == GPT_OK && gpt_create(&bare, 0) == GPT_OK);
    for (auto& q : h) CHECK(gpt_fit(q, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    // bit k of `mask`: optional array k is passed (X0 is the one optional input); the int arrays have width 0 here and live apart
    enum { X0, XO, F, VAR_DYN, VVAR_MAP, VVAR_DYN, ST_X, ST_Z, ST_A, ST_JVAR, ST_MAP_VAR, ST_STATUS, ST_PASSES, ST_RES, ST_DET, N_OPT };
    const size_t width[N_OPT] = {3, 3, 3, 1, 3, 3, 3, 3, 9, 3, 1, 0, 0, 1, 1};
    struct Arrays {
        D y, vel;
        Arr<int> status, st_status, st_passes;
        std::vector<D> opt;
        Arrays(int64_t M, int K, const size_t* w)
            : y(ramp(M * 3)), vel(M * 3, SENT), status(M, ISENT), st_status((size_t)K * M, ISENT), st_passes((size_t)K * M, ISENT) {
            for (int k = 0; k < N_OPT; ++k) opt.push_back(k == X0 ? ramp(M * w[k]) : D((k >= ST_X ? (size_t)K : 1) * M * w[k], SENT));
        }
    };
    auto stages_of = [&](int K) {
        std::vector<gpt_chain_stage> st(K);
        for (int k = 0; k < K; ++k) st[k] = gpt_chain_stage{h[k], R.p, c_src.p, c_dst.p, R.p, 1.0 + 0.25 * k};
        return st;
    };
    auto call = [&](const gpt_chain_stage* st, int K, gpt_handle* hdyn, Arrays& a, int64_t M, int mask, const double* y, double* vel, int* status,
                    double rtol = 1e-10, int max_passes = 50) {
        double* p[N_OPT];
        for (int k = 0; k < N_OPT; ++k) p[k] = (mask >> k & 1) ? a.opt[k].p : nullptr;
        return gpt_pullback_chain(st, K, hdyn, y, p[X0], M, rtol, max_passes, 0.1, p[XO], vel, p[F], status, p[VAR_DYN], p[VVAR_MAP], p[VVAR_DYN],
                                  p[ST_X], p[ST_Z], p[ST_A], p[ST_JVAR], p[ST_MAP_VAR], (mask >> ST_STATUS & 1) ? a.st_status.p : nullptr,
                                  (mask >> ST_PASSES & 1) ? a.st_passes.p : nullptr, p[ST_RES], p[ST_DET]);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.vel.all(SENT) && a.status.all(ISENT) && a.st_status.all(ISENT) && a.st_passes.all(ISENT));
        for (int k = 1; k < N_OPT; ++k) CHECK(a.opt[k].all(SENT));
    };
    const int ALL = (1 << N_OPT) - 1;
    {
        Arrays a(1, 2, width);
        auto st = stages_of(2);
        begin("gpt_pullback_chain refuses K = 0"); done_held(call(st.data(), 0, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses K = 5"); done_held(call(st.data(), GPT_CHAIN_MAX + 1, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses stages = NULL"); done_held(call(nullptr, 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses a NULL dynamics handle"); done_held(call(st.data(), 2, nullptr, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses a dynamics handle without a model"); done_held(call(st.data(), 2, bare, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_STATE);
        auto bad = st; bad[0].h = nullptr;
        begin("gpt_pullback_chain refuses a NULL stage handle"); done_held(call(bad.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        bad = st; bad[0].h = bare;
        begin("gpt_pullback_chain refuses a stage handle without a model"); done_held(call(bad.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_STATE);
        bad = st; bad[1].c_dst = nullptr;
        begin("gpt_pullback_chain refuses a NULL affine pointer"); done_held(call(bad.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        bad = st; bad[1].h = st[0].h;
        begin("gpt_pullback_chain refuses one stage handle twice"); done_held(call(bad.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses a stage handle as the dynamics"); done_held(call(st.data(), 2, st[0].h, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses y = NULL"); done_held(call(st.data(), 2, hd, a, 1, ALL, nullptr, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses vel = NULL"); done_held(call(st.data(), 2, hd, a, 1, ALL, a.y.p, nullptr, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses status = NULL"); done_held(call(st.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, nullptr), GPT_E_ARG);
        begin("gpt_pullback_chain refuses M = -1"); done_held(call(st.data(), 2, hd, a, -1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain refuses rtol = NaN"); done_held(call(st.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p, std::nan("")), GPT_E_ARG);
        begin("gpt_pullback_chain refuses max_passes = 0"); done_held(call(st.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p, 1e-10, 0), GPT_E_ARG);
        D nan_y{0.5, std::nan(""), 0.5};
        begin("gpt_pullback_chain refuses NaN in y"); done_held(call(st.data(), 2, hd, a, 1, ALL, nan_y.p, a.vel.p, a.status.p), GPT_E_ARG);
        bad = st; bad[1].scale = std::nan("");
        begin("gpt_pullback_chain refuses a NaN scale"); done_held(call(bad.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        begin("gpt_pullback_chain M = 0 does nothing"); done_held(call(st.data(), 2, hd, a, 0, ALL, a.y.p, a.vel.p, a.status.p), GPT_OK);
        untouched(a);
    }
    // every optional array on and off: none, all, each one alone, all but each one, at K = 1, 2, 4 (the owner of scratch and staging
    // changes with K); then the staging arithmetic of the stage-major arrays around HOST_CHUNK
    std::vector<int> masks{0, ALL};
    for (int k = 0; k < N_OPT; ++k) { masks.push_back(1 << k); masks.push_back(ALL & ~(1 << k)); }
    for (int K : {1, 2, GPT_CHAIN_MAX}) {
        auto st = stages_of(K);
        for (int64_t M : {(int64_t)1, (int64_t)3, HOST_CHUNK + 1, 2 * HOST_CHUNK + 3})       // growing; the last two walk both staging sets
            for (int mask : masks) {
                if (M > 3 && (K != 2 || (mask != ALL && mask != 0))) continue;
                begin("gpt_pullback_chain K=" + std::to_string(K) + " M=" + std::to_string(M) + " optional=" + std::to_string(mask));
                Arrays a(M, K, width);
                const int rc = call(st.data(), K, hd, a, M, mask, a.y.p, a.vel.p, a.status.p);
                CHECK(stub_live_objects >= held);                        // staging, scratch and events are kept and regrown, never dropped
                held = stub_live_objects;
                done_held(rc, GPT_OK);
                CHECK(a.vel.all(0.0) && a.status.all(0));
                CHECK(a.st_status.all(mask >> ST_STATUS & 1 ? 0 : ISENT) && a.st_passes.all(mask >> ST_PASSES & 1 ? 0 : ISENT));
                for (int k = 1; k < N_OPT; ++k) CHECK(a.opt[k].all(mask >> k & 1 ? 0.0 : SENT));
            }
    }
    {
        begin("gpt_pullback_chain refuses models of different dimension");
        D X2 = ramp(Nd * 2), Y2 = ramp(Nd * 2, 0.01, 0.01), ls2{0.5, 0.75};
        CHECK(gpt_fit(hd, X2.p, Y2.p, Nd, 2, 2, ls2.p, 2, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        Arrays a(1, 2, width);
        auto st = stages_of(2);
        done_held(call(st.data(), 2, hd, a, 1, ALL, a.y.p, a.vel.p, a.status.p), GPT_E_ARG);
        untouched(a);
    }
    begin("gpt_pullback_chain teardown");
    for (auto& q : h) gpt_destroy(q);
    gpt_destroy(hd);
    gpt_destroy(bare);
    done(GPT_OK, GPT_OK);
}

// ---- rollout (gpt_rollout_host.hip): K + 1 handles (K = 0: the dynamics alone), trajectory-major arrays whose rows grow with T, chunks of
// max(1, 131072 / (T + 1)) trajectories through the owner's two staging sets, the launches of a chunk cut every
// GPT_ROLLOUT_STEPS_PER_LAUNCH steps
void rollout_cases() {
    const int64_t N = 5, Nd = 7;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h[GPT_CHAIN_MAX] = {}, *hd = nullptr, *bare = nullptr;
    begin("gpt_rollout_policy setup");
    for (auto& q : h) CHECK(gpt_create(&q, 0) == GPT_OK);
    CHECK(gpt_create(&hd, 0) == GPT_OK && gpt_create(&bare, 0) == GPT_OK);
    for (auto& q : h) CHECK(gpt_fit(q, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    constexpr int X0 = 1, VEL = 2, XO = 4, ALL = 7;     // bits of `mask`: the optional arrays passed
    struct Arrays {
        D y0, x0, path, vel, x;
        Arr<int> steps, status;
        Arrays(int64_t M, int64_t T)
            : y0(ramp(M * 3)), x0(ramp(M * 3)), path((size_t)M * (T + 1) * 3, SENT), vel((size_t)M * T * 3, SENT), x((size_t)M * T * 3, SENT),
              steps(M, ISENT), status(M, ISENT) {}
    };
    auto stages_of = [&](int K) {
        std::vector<gpt_chain_stage> st(K);
        for (int k = 0; k < K; ++k) st[k] = gpt_chain_stage{h[k], R.p, c_src.p, c_dst.p, R.p, 1.0 + 0.25 * k};
        return st;
    };
    auto call = [&](const gpt_chain_stage* st, int K, gpt_handle* hdyn, Arrays& a, int64_t M, int64_t T, int mask, const double* y0, double* path,
                    double dt = 0.5, double rtol = 1e-10, int max_passes = 50) {
        return gpt_rollout_policy(st, K, hdyn, y0, mask & X0 ? a.x0.p : nullptr, M, T, dt, rtol, max_passes, path, mask & VEL ? a.vel.p : nullptr,
                                  mask & XO ? a.x.p : nullptr, a.steps.p, a.status.p);
    };
    auto untouched = [&](const Arrays& a) { CHECK(a.path.all(SENT) && a.vel.all(SENT) && a.x.all(SENT) && a.steps.all(ISENT) && a.status.all(ISENT)); };
    {
        Arrays a(1, 2);
        auto st = stages_of(2);
        begin("gpt_rollout_policy refuses K = -1"); done_held(call(st.data(), -1, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses K = 5"); done_held(call(st.data(), GPT_CHAIN_MAX + 1, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses stages = NULL with K = 2"); done_held(call(nullptr, 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses a NULL dynamics handle"); done_held(call(st.data(), 2, nullptr, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses a dynamics handle without a model, K = 0"); done_held(call(nullptr, 0, bare, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_STATE);
        auto bad = st; bad[0].h = bare;
        begin("gpt_rollout_policy refuses a stage handle without a model"); done_held(call(bad.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_STATE);
        bad = st; bad[1].h = st[0].h;
        begin("gpt_rollout_policy refuses one stage handle twice"); done_held(call(bad.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses n_steps = -1"); done_held(call(st.data(), 2, hd, a, 1, -1, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses dt = 0"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p, 0.0), GPT_E_ARG);
        begin("gpt_rollout_policy refuses dt = inf"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p, INFINITY), GPT_E_ARG);
        begin("gpt_rollout_policy refuses dt = NaN"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p, std::nan("")), GPT_E_ARG);
        begin("gpt_rollout_policy refuses rtol = 0"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p, 0.5, 0.0), GPT_E_ARG);
        begin("gpt_rollout_policy refuses max_passes = 0"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p, 0.5, 1e-10, 0), GPT_E_ARG);
        begin("gpt_rollout_policy refuses M = -1"); done_held(call(st.data(), 2, hd, a, -1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        // M (T + 1) at the limit, cut either way: 2^31 rows are refused before anything is sized
        begin("gpt_rollout_policy refuses M (T + 1) = 2^31, M = 2^15"); done_held(call(st.data(), 2, hd, a, 1 << 15, (1 << 16) - 1, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses M (T + 1) = 2^31, M = 1"); done_held(call(st.data(), 2, hd, a, 1, ((int64_t)1 << 31) - 1, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses M (T + 1) = 2^31, T = 0"); done_held(call(st.data(), 2, hd, a, (int64_t)1 << 31, 0, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses y0 = NULL"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, nullptr, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy refuses path = NULL"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, nullptr), GPT_E_ARG);
        D nan_y{0.5, std::nan(""), 0.5};
        begin("gpt_rollout_policy refuses NaN in y0"); done_held(call(st.data(), 2, hd, a, 1, 2, ALL, nan_y.p, a.path.p), GPT_E_ARG);
        bad = st; bad[1].scale = std::nan("");
        begin("gpt_rollout_policy refuses a NaN scale"); done_held(call(bad.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        begin("gpt_rollout_policy M = 0 does nothing"); done_held(call(st.data(), 2, hd, a, 0, 2, ALL, a.y0.p, a.path.p), GPT_OK);
        untouched(a);
    }
    // (M, T, steps per launch): T = 0; one trajectory; launches cut inside a call and at its last step; T = 255: chunks of 512, M one past
    // one and past two of them; T = 131071: chunks of 1, three of them
    struct Shape { int64_t M, T; int per; };
    const Shape shapes[] = {{1, 0, 256}, {3, 0, 256}, {1, 1, 256}, {3, 7, 3}, {3, 6, 3}, {2, 300, 256}, {513, 255, 256}, {1027, 255, 100}, {3, 131071, 65536}};
    for (int K : {0, 1, 2, GPT_CHAIN_MAX}) {
        auto st = stages_of(K);
        for (const Shape& sh : shapes)
            for (int mask : {0, ALL, X0 | XO, VEL}) {
                if (sh.M > 3 && (K != 2 || (mask != ALL && mask != 0))) continue;
                if (sh.T > 1000 && (K != 0 || mask != ALL)) continue;
                begin("gpt_rollout_policy K=" + std::to_string(K) + " M=" + std::to_string(sh.M) + " T=" + std::to_string(sh.T) + " steps per launch=" +
                      std::to_string(sh.per) + " optional=" + std::to_string(mask));
                setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", std::to_string(sh.per).c_str(), 1);
                gpt::stub_rollout_launch_count = 0;
                Arrays a(sh.M, sh.T);
                const int rc = call(K ? st.data() : nullptr, K, hd, a, sh.M, sh.T, mask, a.y0.p, a.path.p);
                CHECK(stub_live_objects >= held);                        // staging, scratch and events are kept and regrown, never dropped
                held = stub_live_objects;
                done_held(rc, GPT_OK);
                const int64_t chunk = std::max<int64_t>(1, 131072 / (sh.T + 1)), chunks = (sh.M + chunk - 1) / chunk;
                CHECK(gpt::stub_rollout_launch_count == chunks * std::max<int64_t>(1, (sh.T + sh.per - 1) / sh.per));
                CHECK(a.path.all(0.0) && a.status.all(0) && a.steps.all((int)sh.T));
                CHECK(a.vel.all(mask & VEL ? 0.0 : SENT) && a.x.all(mask & XO ? 0.0 : SENT));
            }
    }
    unsetenv("GPT_ROLLOUT_STEPS_PER_LAUNCH");
    {
        begin("gpt_rollout_policy refuses models of different dimension");
        D X2 = ramp(Nd * 2), Y2 = ramp(Nd * 2, 0.01, 0.01), ls2{0.5, 0.75};
        CHECK(gpt_fit(hd, X2.p, Y2.p, Nd, 2, 2, ls2.p, 2, 1.0, 0.01, 1e-10) == GPT_OK);
        held = stub_live_objects;
        Arrays a(1, 2);
        auto st = stages_of(2);
        done_held(call(st.data(), 2, hd, a, 1, 2, ALL, a.y0.p, a.path.p), GPT_E_ARG);
        untouched(a);
    }
    begin("gpt_rollout_policy teardown");
    for (auto& q : h) gpt_destroy(q);
    gpt_destroy(hd);
    gpt_destroy(bare);
    done(GPT_OK, GPT_OK);
}

// ---- stabilised rollout (gpt_rollout_stab_host.hip): the arrays of the rollout and f, dvar (rows of T D doubles) and var (rows of T
// doubles: the one array of the table whose rows have no factor D); chunks and launches as the rollout's, 32 steps per launch unless set
void rollout_stab_cases() {
    const int64_t N = 5, Nd = 7;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h[2] = {}, *hd = nullptr, *m12 = nullptr, *m32 = nullptr;
    begin("gpt_rollout_stabilised setup");
    for (auto& q : h) CHECK(gpt_create(&q, 0) == GPT_OK);
    CHECK(gpt_create(&hd, 0) == GPT_OK && gpt_create(&m12, 0) == GPT_OK && gpt_create(&m32, 0) == GPT_OK);
    for (auto& q : h) CHECK(gpt_fit(q, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit_kernel(m12, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10, GPT_KERNEL_MATERN12) == GPT_OK);
    CHECK(gpt_fit_kernel(m32, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10, GPT_KERNEL_MATERN32) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    constexpr int X0 = 1, VEL = 2, XO = 4, F = 8, VAR = 16, DVAR = 32, ALL = 63;     // bits of `mask`: the optional arrays passed
    struct Arrays {
        D y0, x0, path, vel, x, f, var, dvar;
        Arr<int> steps, status;
        Arrays(int64_t M, int64_t T)
            : y0(ramp(M * 3)), x0(ramp(M * 3)), path((size_t)M * (T + 1) * 3, SENT), vel((size_t)M * T * 3, SENT), x((size_t)M * T * 3, SENT),
              f((size_t)M * T * 3, SENT), var((size_t)M * T, SENT), dvar((size_t)M * T * 3, SENT), steps(M, ISENT), status(M, ISENT) {}
    };
    std::vector<gpt_chain_stage> st2{gpt_chain_stage{h[0], R.p, c_src.p, c_dst.p, R.p, 1.0}, gpt_chain_stage{h[1], R.p, c_src.p, c_dst.p, R.p, 1.25}};
    auto call = [&](const gpt_chain_stage* st, int K, gpt_handle* hdyn, Arrays& a, int64_t M, int64_t T, int mask, double gain = 1.0,
                    double off = 0.1) {
        return gpt_rollout_stabilised(st, K, hdyn, a.y0.p, mask & X0 ? a.x0.p : nullptr, M, T, 0.5, 1e-10, 50, gain, off, a.path.p,
                                      mask & VEL ? a.vel.p : nullptr, mask & XO ? a.x.p : nullptr, mask & F ? a.f.p : nullptr,
                                      mask & VAR ? a.var.p : nullptr, mask & DVAR ? a.dvar.p : nullptr, a.steps.p, a.status.p);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.path.all(SENT) && a.vel.all(SENT) && a.x.all(SENT) && a.f.all(SENT) && a.var.all(SENT) && a.dvar.all(SENT) && a.steps.all(ISENT) &&
              a.status.all(ISENT));
    };
    {
        Arrays a(1, 2);
        begin("gpt_rollout_stabilised refuses gain = -1"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, -1.0), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses gain = NaN"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, std::nan("")), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses gain = inf"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, INFINITY), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses std_offset = NaN"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, 1.0, std::nan("")), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses a Matern 1/2 dynamics"); done_held(call(nullptr, 0, m12, a, 1, 2, ALL), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses a Matern 3/2 dynamics without its derivatives"); done_held(call(st2.data(), 2, m32, a, 1, 2, ALL), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses n_steps = -1"); done_held(call(st2.data(), 2, hd, a, 1, -1, ALL), GPT_E_ARG);
        begin("gpt_rollout_stabilised refuses stages = NULL with K = 2"); done_held(call(nullptr, 2, hd, a, 1, 2, ALL), GPT_E_ARG);
        begin("gpt_rollout_stabilised M = 0 does nothing"); done_held(call(st2.data(), 2, hd, a, 0, 2, ALL), GPT_OK);
        untouched(a);
    }
    CHECK(gpt_set_matern_derivatives(m32, 1) == GPT_OK);
    // (M, T, steps per launch): T = 0 (the per-step arrays have no rows); one chunk, launches cut inside it and at its last step; T = 255:
    // chunks of 512, M one past one and past two of them
    struct Shape { int64_t M, T; int per; };
    const Shape shapes[] = {{1, 0, 0}, {3, 0, 0}, {1, 1, 0}, {3, 7, 3}, {3, 6, 3}, {2, 70, 0}, {513, 255, 0}, {1027, 255, 100}};
    // the optional arrays: none, all, var without dvar, dvar without var, f and vel alone
    for (int K : {0, 2}) {
        for (gpt_handle* dyn : {hd, m32})
            for (const Shape& sh : shapes)
                for (int mask : {0, ALL, X0 | VAR, XO | DVAR, VEL | F}) {
                    if (sh.M > 3 && (K != 2 || dyn != hd || (mask != ALL && mask != (X0 | VAR)))) continue;
                    begin("gpt_rollout_stabilised K=" + std::to_string(K) + (dyn == hd ? " RBF" : " Matern 3/2") + " M=" + std::to_string(sh.M) + " T=" +
                          std::to_string(sh.T) + " steps per launch=" + std::to_string(sh.per) + " optional=" + std::to_string(mask));
                    if (sh.per) setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", std::to_string(sh.per).c_str(), 1);
                    else unsetenv("GPT_ROLLOUT_STEPS_PER_LAUNCH");
                    const int per = sh.per ? sh.per : 32;                      // ROLLOUT_STAB_STEPS_PER_LAUNCH
                    gpt::stub_rollout_launch_count = 0;
                    Arrays a(sh.M, sh.T);
                    const int rc = call(K ? st2.data() : nullptr, K, dyn, a, sh.M, sh.T, mask);      // K = 0: stages == NULL
                    CHECK(stub_live_objects >= held);                        // staging, scratch and events are kept and regrown, never dropped
                    held = stub_live_objects;
                    done_held(rc, GPT_OK);
                    const int64_t chunk = std::max<int64_t>(1, 131072 / (sh.T + 1)), chunks = (sh.M + chunk - 1) / chunk;
                    CHECK(gpt::stub_rollout_launch_count == chunks * std::max<int64_t>(1, (sh.T + per - 1) / per));
                    CHECK(a.path.all(0.0) && a.status.all(0) && a.steps.all((int)sh.T));
                    CHECK(a.vel.all(mask & VEL ? 0.0 : SENT) && a.x.all(mask & XO ? 0.0 : SENT) && a.f.all(mask & F ? 0.0 : SENT));
                    CHECK(a.var.all(mask & VAR ? 0.0 : SENT) && a.dvar.all(mask & DVAR ? 0.0 : SENT));
                }
    }
    unsetenv("GPT_ROLLOUT_STEPS_PER_LAUNCH");
    begin("gpt_rollout_stabilised teardown");
    for (auto& q : h) gpt_destroy(q);
    gpt_destroy(hd);
    gpt_destroy(m12);
    gpt_destroy(m32);
    done(GPT_OK, GPT_OK);
}

// ---- sampled rollout (gpt_rollout_sampled_host.hip): three inputs (y0, x0, normals: rows of T D doubles), the arrays of the rollout
// and f (T D), pvar, cvar (T) and chol (T T doubles per path); chunks as the rollout's and further held to the paths whose device
// scratch fits the budget (GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES), sixteen at the least
void rollout_sampled_cases() {
    const int64_t N = 5, Nd = 7;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h[2] = {}, *hd = nullptr, *m12 = nullptr;
    begin("gpt_rollout_sampled setup");
    for (auto& q : h) CHECK(gpt_create(&q, 0) == GPT_OK);
    CHECK(gpt_create(&hd, 0) == GPT_OK && gpt_create(&m12, 0) == GPT_OK);
    for (auto& q : h) CHECK(gpt_fit(q, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit_kernel(m12, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10, GPT_KERNEL_MATERN12) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    constexpr int X0 = 1, VEL = 2, XO = 4, F = 8, PVAR = 16, CVAR = 32, CHOL = 64, ALL = 127;     // bits of `mask`: the optional arrays passed
    struct Arrays {
        D y0, x0, z, path, vel, x, f, pvar, cvar, chol;
        Arr<int> steps, status;
        Arrays(int64_t M, int64_t T)
            : y0(ramp(M * 3)), x0(ramp(M * 3)), z(ramp(M * T * 3, 0.0, 1e-3)), path((size_t)M * (T + 1) * 3, SENT), vel((size_t)M * T * 3, SENT),
              x((size_t)M * T * 3, SENT), f((size_t)M * T * 3, SENT), pvar((size_t)M * T, SENT), cvar((size_t)M * T, SENT),
              chol((size_t)M * T * T, SENT), steps(M, ISENT), status(M, ISENT) {}
    };
    std::vector<gpt_chain_stage> st2{gpt_chain_stage{h[0], R.p, c_src.p, c_dst.p, R.p, 1.0}, gpt_chain_stage{h[1], R.p, c_src.p, c_dst.p, R.p, 1.25}};
    auto call = [&](const gpt_chain_stage* st, int K, gpt_handle* hdyn, Arrays& a, int64_t M, int64_t T, int mask, double nugget = 0.01,
                    const double* z = nullptr, bool no_z = false) {
        return gpt_rollout_sampled(st, K, hdyn, a.y0.p, mask & X0 ? a.x0.p : nullptr, no_z ? nullptr : (z ? z : a.z.p), M, T, 0.5, 1e-10, 50, nugget,
                                   a.path.p, mask & VEL ? a.vel.p : nullptr, mask & XO ? a.x.p : nullptr, mask & F ? a.f.p : nullptr,
                                   mask & PVAR ? a.pvar.p : nullptr, mask & CVAR ? a.cvar.p : nullptr, mask & CHOL ? a.chol.p : nullptr, a.steps.p,
                                   a.status.p);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.path.all(SENT) && a.vel.all(SENT) && a.x.all(SENT) && a.f.all(SENT) && a.pvar.all(SENT) && a.cvar.all(SENT) && a.chol.all(SENT) &&
              a.steps.all(ISENT) && a.status.all(ISENT));
    };
    {
        Arrays a(1, 2);
        begin("gpt_rollout_sampled refuses nugget = -1"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, -1.0), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses nugget = NaN"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, std::nan("")), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses nugget = inf"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, INFINITY), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses n_steps = 257"); done_held(call(st2.data(), 2, hd, a, 1, GPT_ROLLOUT_SAMPLED_MAX_T + 1, ALL), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses n_steps = -1"); done_held(call(st2.data(), 2, hd, a, 1, -1, ALL), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses normals = NULL"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, 0.01, nullptr, true), GPT_E_ARG);
        D nan_z{0.5, 0.5, 0.5, 0.5, std::nan(""), 0.5};
        begin("gpt_rollout_sampled refuses NaN in normals"); done_held(call(st2.data(), 2, hd, a, 1, 2, ALL, 0.01, nan_z.p), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses stages = NULL with K = 2"); done_held(call(nullptr, 2, hd, a, 1, 2, ALL), GPT_E_ARG);
        begin("gpt_rollout_sampled refuses P (T + 1) = 2^31"); done_held(call(st2.data(), 2, hd, a, (int64_t)1 << 23, 255, ALL), GPT_E_ARG);
        begin("gpt_rollout_sampled M = 0 does nothing"); done_held(call(st2.data(), 2, hd, a, 0, 2, ALL), GPT_OK);
        untouched(a);
    }
    // (M, T, steps per launch, scratch budget in bytes or 0): T = 0 (the per-step arrays have no rows, normals may be NULL), 1 and the
    // largest; launches cut inside a call and at its last step; a budget of one byte: chunks of sixteen paths, M at the chunk boundary,
    // one short of it and one past it, and past two chunks
    struct Shape { int64_t M, T; int per; long budget; };
    // (the steps per launch are always set: the call's default is a measured constant of gpt_rollout_sampled.h, not this driver's business)
    const Shape shapes[] = {{1, 0, 300, 0}, {3, 0, 300, 0}, {1, 1, 300, 0}, {3, 7, 3, 0}, {3, 6, 3, 0}, {2, GPT_ROLLOUT_SAMPLED_MAX_T, 300, 0},
                            {2, GPT_ROLLOUT_SAMPLED_MAX_T, 100, 0}, {15, 5, 300, 1}, {16, 5, 300, 1}, {17, 5, 2, 1}, {33, 5, 300, 1}, {513, 255, 128, 0}};
    // the optional arrays: none, all, each alone, and all but each
    std::vector<int> masks{0, ALL};
    for (int bit = 1; bit < ALL; bit <<= 1) { masks.push_back(bit); masks.push_back(ALL & ~bit); }
    for (int K : {0, 2}) {
        for (gpt_handle* dyn : {hd, m12})
            for (const Shape& sh : shapes)
                for (int mask : masks) {
                    if ((sh.M > 3 || sh.T > 7) && (mask != ALL && mask != 0 && mask != (ALL & ~XO))) continue;
                    if (sh.M > 33 && (K != 2 || dyn != hd || mask != ALL)) continue;
                    begin("gpt_rollout_sampled K=" + std::to_string(K) + (dyn == hd ? " RBF" : " Matern 1/2") + " M=" + std::to_string(sh.M) + " T=" +
                          std::to_string(sh.T) + " steps per launch=" + std::to_string(sh.per) + " budget=" + std::to_string(sh.budget) + " optional=" +
                          std::to_string(mask));
                    setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", std::to_string(sh.per).c_str(), 1);
                    if (sh.budget) setenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES", std::to_string(sh.budget).c_str(), 1);
                    else unsetenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES");
                    const int per = sh.per;
                    gpt::stub_rollout_launch_count = 0;
                    Arrays a(sh.M, sh.T);
                    const int rc = call(K ? st2.data() : nullptr, K, dyn, a, sh.M, sh.T, mask, 0.01, nullptr, sh.T == 0);
                    CHECK(stub_live_objects >= held);                        // staging, scratch and events are kept and regrown, never dropped
                    held = stub_live_objects;
                    done_held(rc, GPT_OK);
                    int64_t chunk = std::max<int64_t>(1, 131072 / (sh.T + 1));
                    if (sh.budget) chunk = std::min<int64_t>(chunk, 16);
                    const int64_t chunks = (sh.M + chunk - 1) / chunk;
                    CHECK(gpt::stub_rollout_launch_count == chunks * std::max<int64_t>(1, (sh.T + per - 1) / per));
                    CHECK(a.path.all(0.0) && a.status.all(0) && a.steps.all((int)sh.T));
                    CHECK(a.vel.all(mask & VEL ? 0.0 : SENT) && a.x.all(mask & XO ? 0.0 : SENT) && a.f.all(mask & F ? 0.0 : SENT));
                    CHECK(a.pvar.all(mask & PVAR ? 0.0 : SENT) && a.cvar.all(mask & CVAR ? 0.0 : SENT) && a.chol.all(mask & CHOL ? 0.0 : SENT));
                }
    }
    unsetenv("GPT_ROLLOUT_STEPS_PER_LAUNCH");
    unsetenv("GPT_ROLLOUT_SAMPLED_SCRATCH_BYTES");
    begin("gpt_rollout_sampled teardown");
    for (auto& q : h) gpt_destroy(q);
    gpt_destroy(hd);
    gpt_destroy(m12);
    done(GPT_OK, GPT_OK);
}

// ---- pathwise rollout (gpt_rollout_pathwise_host.hip): three per-path inputs (y0, x0, func: an int per path), the arrays of the
// rollout and f; what the functions bring has no row per path and is uploaded once: the weights (S,N,D) packed into images
// [S][NP][4], omega (J,D), amp (S,J,2,D), each at its exact size; chunks as the rollout's, or GPT_ROLLOUT_PATHWISE_CHUNK paths
void rollout_pathwise_cases() {
    const int64_t N = 5, Nd = 7;
    D X = ramp(N * 3), Y = ramp(N * 3, 0.01, 0.01), Xd = ramp(Nd * 3), Yd = ramp(Nd * 3, 0.02, 0.01), ls{0.5, 0.75, 0.6};
    D R{1, 0, 0, 0, 1, 0, 0, 0, 1}, c_src{0.1, 0.2, 0.3}, c_dst{0.3, 0.2, 0.1};
    gpt_handle *h[2] = {}, *hd = nullptr;
    begin("gpt_rollout_pathwise setup");
    for (auto& q : h) CHECK(gpt_create(&q, 0) == GPT_OK);
    CHECK(gpt_create(&hd, 0) == GPT_OK);
    for (auto& q : h) CHECK(gpt_fit(q, X.p, Y.p, N, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    CHECK(gpt_fit(hd, Xd.p, Yd.p, Nd, 3, 3, ls.p, 3, 1.0, 0.01, 1e-10) == GPT_OK);
    long held = stub_live_objects;
    auto done_held = [&](int rc, int want) {
        CHECK(rc == want);
        CHECK(stub_live_objects == held);
        printf("ok  %s\n", g_case.c_str());
        ++g_cases;
    };
    struct Arrays {
        D y0, x0, path, vel, x, f, w, omega, amp;
        Arr<int> func, steps, status;
        Arrays(int64_t M, int64_t T, int64_t S, int64_t J, int64_t Nd_)
            : y0(ramp(M * 3)), x0(ramp(M * 3)), path((size_t)M * (T + 1) * 3, SENT), vel((size_t)M * T * 3, SENT), x((size_t)M * T * 3, SENT),
              f((size_t)M * T * 3, SENT), w(ramp(S * Nd_ * 3)), omega(ramp(J * 3)), amp(ramp(S * J * 6)), func(M, 0), steps(M, ISENT),
              status(M, ISENT) {
            for (int64_t m = 0; m < M; ++m) func.p[m] = (int)((m * 5 + 1) % S);
        }
    };
    std::vector<gpt_chain_stage> st2{gpt_chain_stage{h[0], R.p, c_src.p, c_dst.p, R.p, 1.0}, gpt_chain_stage{h[1], R.p, c_src.p, c_dst.p, R.p, 1.25}};
    constexpr int X0 = 1, VEL = 2, XO = 4, FO = 8, ALL = 15;
    auto call = [&](const gpt_chain_stage* st, int K, Arrays& a, int64_t M, int64_t T, int64_t S, int64_t J, int mask, const int* func,
                    const double* w, const double* om, const double* amp) {
        return gpt_rollout_pathwise(st, K, hd, a.y0.p, mask & X0 ? a.x0.p : nullptr, func, M, T, 0.5, 1e-10, 50, S, w, J, om, amp, a.path.p,
                                    mask & VEL ? a.vel.p : nullptr, mask & XO ? a.x.p : nullptr, mask & FO ? a.f.p : nullptr, a.steps.p, a.status.p);
    };
    auto untouched = [&](const Arrays& a) {
        CHECK(a.path.all(SENT) && a.vel.all(SENT) && a.x.all(SENT) && a.f.all(SENT) && a.steps.all(ISENT) && a.status.all(ISENT));
    };
    {
        Arrays a(2, 2, 3, 4, Nd);
        const gpt_chain_stage* st = st2.data();
        begin("gpt_rollout_pathwise refuses S = 0"); done_held(call(st, 2, a, 2, 2, 0, 4, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses J = -1"); done_held(call(st, 2, a, 2, 2, 3, -1, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses J = 8193");
        done_held(call(st, 2, a, 2, 2, 3, GPT_PATHWISE_MAX_FREQ + 1, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses func = NULL"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, nullptr, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses weights = NULL"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, nullptr, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses omega = NULL with J > 0"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, a.w.p, nullptr, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses amp = NULL with J > 0"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, a.w.p, a.omega.p, nullptr), GPT_E_ARG);
        Arr<int> bad_f{0, 3}, neg_f{-1, 0};
        begin("gpt_rollout_pathwise refuses func = S"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, bad_f.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses func = -1"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, neg_f.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        D nan_w(a.w), nan_o(a.omega), nan_a(a.amp);
        nan_w.p[nan_w.n - 1] = std::nan(""); nan_o.p[nan_o.n - 1] = INFINITY; nan_a.p[nan_a.n - 1] = std::nan("");
        begin("gpt_rollout_pathwise refuses NaN in weights"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, nan_w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses infinity in omega"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, a.w.p, nan_o.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses NaN in amp"); done_held(call(st, 2, a, 2, 2, 3, 4, ALL, a.func.p, a.w.p, a.omega.p, nan_a.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses n_steps = -1"); done_held(call(st, 2, a, 2, -1, 3, 4, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise refuses stages = NULL with K = 2"); done_held(call(nullptr, 2, a, 2, 2, 3, 4, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_E_ARG);
        begin("gpt_rollout_pathwise M = 0 does nothing"); done_held(call(st, 2, a, 0, 2, 3, 4, ALL, a.func.p, a.w.p, a.omega.p, a.amp.p), GPT_OK);
        untouched(a);
    }
    // (M, T, S, J, steps per launch, paths per chunk or 0): J = 0 without omega and amp; one function; M S no multiple of the chunk,
    // one path past one and past two chunks; T = 0; launches cut inside a call
    struct Shape { int64_t M, T, S, J; int per; int64_t chunk; };
    const Shape shapes[] = {{1, 0, 1, 0, 32, 0}, {3, 1, 1, 0, 32, 0}, {3, 7, 2, 1, 3, 0}, {5, 6, 3, 65, 3, 4}, {9, 7, 3, 64, 32, 4}, {7, 40, 4, 130, 32, 3},
                            {513, 255, 2, 3, 256, 0}};
    for (int K : {0, 2})
        for (const Shape& sh : shapes)
            for (int mask : {0, ALL, X0 | XO, VEL | FO}) {
                if (sh.M > 9 && (K != 2 || mask != ALL)) continue;
                begin("gpt_rollout_pathwise K=" + std::to_string(K) + " M=" + std::to_string(sh.M) + " T=" + std::to_string(sh.T) + " S=" + std::to_string(sh.S) +
                      " J=" + std::to_string(sh.J) + " steps per launch=" + std::to_string(sh.per) + " chunk=" + std::to_string(sh.chunk) + " optional=" +
                      std::to_string(mask));
                setenv("GPT_ROLLOUT_STEPS_PER_LAUNCH", std::to_string(sh.per).c_str(), 1);
                if (sh.chunk) setenv("GPT_ROLLOUT_PATHWISE_CHUNK", std::to_string(sh.chunk).c_str(), 1);
                else unsetenv("GPT_ROLLOUT_PATHWISE_CHUNK");
                gpt::stub_rollout_launch_count = 0;
                Arrays a(sh.M, sh.T, sh.S, sh.J, Nd);
                const int rc = call(K ? st2.data() : nullptr, K, a, sh.M, sh.T, sh.S, sh.J, mask, a.func.p, a.w.p, sh.J ? a.omega.p : nullptr,
                                    sh.J ? a.amp.p : nullptr);
                CHECK(stub_live_objects >= held);                        // staging, scratch and events are kept and regrown, never dropped
                held = stub_live_objects;
                done_held(rc, GPT_OK);
                int64_t chunk = std::max<int64_t>(1, 131072 / (sh.T + 1));
                if (sh.chunk) chunk = std::min(chunk, sh.chunk);
                const int64_t chunks = (sh.M + chunk - 1) / chunk;
                CHECK(gpt::stub_rollout_launch_count == chunks * std::max<int64_t>(1, (sh.T + sh.per - 1) / sh.per));
                CHECK(a.path.all(0.0) && a.status.all(0) && a.steps.all((int)sh.T));
                CHECK(a.vel.all(mask & VEL ? 0.0 : SENT) && a.x.all(mask & XO ? 0.0 : SENT) && a.f.all(mask & FO ? 0.0 : SENT));
            }
    unsetenv("GPT_ROLLOUT_STEPS_PER_LAUNCH");
    unsetenv("GPT_ROLLOUT_PATHWISE_CHUNK");
    {
        // gpt_apply_inverse (gpt_api.hip): the columns of a call in passes of four, the last one padded; R and out at their exact sizes
        for (int64_t C : {1, 4, 5, 9}) {
            begin("gpt_apply_inverse C=" + std::to_string(C));
            D Rh = ramp(Nd * C), out((size_t)(Nd * C), SENT);
            const int rc = gpt_apply_inverse(hd, Rh.p, C, out.p);
            CHECK(stub_live_objects >= held);
            held = stub_live_objects;
            done_held(rc, GPT_OK);
            CHECK(out.all(0.0));
        }
        D Rh = ramp(Nd), out((size_t)Nd, SENT);
        begin("gpt_apply_inverse refuses C = -1"); done_held(gpt_apply_inverse(hd, Rh.p, -1, out.p), GPT_E_ARG);
        begin("gpt_apply_inverse refuses R = NULL"); done_held(gpt_apply_inverse(hd, nullptr, 1, out.p), GPT_E_ARG);
        begin("gpt_apply_inverse C = 0 does nothing"); done_held(gpt_apply_inverse(hd, nullptr, 0, nullptr), GPT_OK);
        CHECK(out.all(SENT));
    }
    begin("gpt_rollout_pathwise teardown");
    for (auto& q : h) gpt_destroy(q);
    gpt_destroy(hd);
    done(GPT_OK, GPT_OK);
}

}  // namespace

int main() {
    const std::vector<int> sizes3{1, 32, 33}, sizes4{128, 2, 32, 33};      // both size classes in one call, each at its edge
    for (auto [Dm, n_ls, O] : {std::array<int, 3>{1, 1, 1}, std::array<int, 3>{3, 3, 3}, std::array<int, 3>{15, 1, 16}}) {
        batch_cases({sizes3, Dm, n_ls, O}, {0, 64, 65}, -1);               // an empty member, a full tile, one query past it
        batch_cases({sizes4, Dm, n_ls, O}, {65, 0, 64, 65}, -1);
    }
    batch_cases({sizes3, 3, 3, 3}, {0, 0, 0}, -1);                         // no query at all
    batch_cases({sizes3, 3, 3, 3}, {65, 64, 65}, 1);                       // the middle member is not positive definite
    batch_cases({sizes4, 15, 1, 16}, {65, 64, 0, 65}, 1);
    batch_refusals();
    batch_opt_cases({{10}, 2, 2, 2}, 1, 1, -1);                            // R = 1
    batch_opt_cases({sizes3, 1, 1, 1}, 5, 3, -1);                          // R odd: both size classes, several slices
    batch_opt_cases({sizes4, 3, 3, 3}, 12, 4, -1);                         // R even
    batch_opt_cases({sizes4, 15, 1, 16}, 7, 2, 1);                         // the runs of one model start where it is not PD
    batch_opt_cases({sizes4, 15, 15, 16}, 9, 5, 0);                        // the largest record; the only large model fails
    batch_opt_refusals();
    batch_opt_bounded_cases({{10}, 2, 2, 2}, 1, 1, -1);                    // R = 1
    batch_opt_bounded_cases({sizes3, 1, 1, 1}, 7, 3, -1);                  // R a multiple of nothing: both size classes, several slices
    batch_opt_bounded_cases({sizes4, 3, 3, 3}, 13, 4, 1);                  // the runs of one model start where it is not PD
    for (int surrogate : {0, 1}) {
        for (auto [Dm, n_ls] : {std::array<int, 2>{1, 1}, std::array<int, 2>{2, 2}, std::array<int, 2>{3, 1}}) {
            fold_scan_cases({sizes3, Dm, n_ls, Dm}, {0, 64, 65}, false, surrogate, -1, -1);     // B odd: an empty member, a full tile, one past it
            fold_scan_cases({sizes4, Dm, n_ls, Dm}, {65, 1, 0, 129}, false, surrogate, -1, -1); // B even
        }
        for (int M : {0, 1, 65}) fold_scan_cases({sizes3, 3, 3, 3}, {M}, true, surrogate, -1, -1);   // shared queries: M = 0, 1, a tile and one
        fold_scan_cases({sizes4, 2, 2, 2}, {129}, true, surrogate, 2, -1);                      // a member that is not positive definite
        fold_scan_cases({sizes4, 3, 3, 3}, {65, 64, 1, 65}, false, surrogate, 0, -1);
    }
    fold_scan_cases({sizes3, 2, 2, 2}, {65}, true, 1, -1, 1);              // the surrogate alone is not positive definite
    fold_scan_cases({sizes4, 3, 1, 3}, {1, 65, 64, 0}, false, 1, 3, 1);    // ... beside a member that is not
    fold_scan_refusals();
    select_cases();
    svgp_cases("gpt_svgp", gpt_svgp_train, gpt_svgp_elbo_grad, false);
    svgp_cases("gpt_svgp_surface", gpt_svgp_surface_train, gpt_svgp_surface_elbo_grad, true);
    surface_predict_cases();
    predict_all_cases<double>(GPT_F64, "fp64");
    predict_all_cases<float>(GPT_F32, "fp32");
    inverse_map_cases();
    transport_cases();
    pullback_cases();
    chain_cases();
    rollout_cases();
    rollout_stab_cases();
    rollout_sampled_cases();
    rollout_pathwise_cases();
    printf("ONESHOT_DRIVER_OK %d cases\n", g_cases);
    return 0;
}
