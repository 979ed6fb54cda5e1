// The hyper-parameter search of a batch of small GPs on the device — gpt_batch_optimize, gpt_batch_optimize_bounded (include/gpt_hip.h).  One workgroup owns
// one RUN, a (model, start point) pair, and carries it through a projected BFGS iteration on f = -LML over theta = log [c, l..,
// noise] inside a box, without returning to the host between objective evaluations:
//     start   x = clip(x0); f, g there; H = I.  Not PD there: GPT_OPT_NOT_PD_START.
//     step    pg = x - clip(x - g): PGTOL if max |pg| <= pgtol; then the caps MAX_ITER, MAX_EVALS
//             active set: fixed components (lo == hi) and those on a bound whose gradient points outward
//             d = -H[free, free] g[free], 0 on the active set; if d.g >= 0: H = I, d = -g on the free set
//             t = 1 (first iteration: min(1, 1 / |d|)); trial xn = clip(x + t d), accepted if f(xn) is finite and
//             f(xn) <= f + 1e-4 g.(xn - x); otherwise t /= 2, at most max_ls times, then LINESEARCH
//             accepted: s = xn - x, y = gn - g (0 on fixed components); BFGS update of H if s.y > 1e-10 |s| |y|;
//             FTOL if f - fn <= ftol max(|f|, |fn|, 1)
// (tests/batch_search_restatement.py states the same iteration in numpy.)  The objective and its gradient come from the function
// bat_factor is built on for gpt_batch_lml_objective (bat_factor_body, bat_lml, bat_grad: gpt_batch_device.h): the whole workgroup
// works on them, in the same size classes, so a run's result does not depend on the batch around it.  Everything else is
// O(P^2) arithmetic, P = 2 + n_ls <= 17, done by thread 0 on the run's record in global memory (gpt_batch_opt.h); the trial point
// reaches the other threads through LDS.
//
// The kernel is a state machine with one transition per objective evaluation: evaluate at the pending trial point, then thread 0
// folds the result into the record and either ends the run or leaves the next trial point pending.  After every transition the
// record alone says where the run stands, so a launch may stop after any number of evaluations (a.evals_per_launch bounds how
// long one launch lasts) and the next one resumes bit for bit where it stopped.  A trial point whose matrix is not PD is a
// rejected step, not an exit: bat_factor_body returns false from every thread at the same pivot, after the same barriers, and
// every barrier of the loop below is reached by all threads or by none.
//
// Device side only: the kernel and the launcher of gpt_batch_opt.h.  The entry point is in gpt_batch_opt_host.hip.
#include "gpt_batch_opt.h"
#include "gpt_batch_device.h"
#include "gpt_dispatch.h"
#include "../../include/gpt_hip.h"

namespace gpt {
namespace {

__device__ __forceinline__ double clip(const double v, const double lo, const double hi) { return fmin(fmax(v, lo), hi); }

// Thread 0, after the evaluation at the trial point th (ok: the matrix was PD; sums: bat_factor_body's): one transition of the
// run's state machine.  Returns whether the run goes on, with the next trial point in th and in the record.
__device__ __forceinline__ bool opt_advance(const BatOptArgs& a, const int r, const int n, const bool ok, const double (&sums)[BAT_RED],
                                            const double c, const double noise, double* __restrict__ th) {
    const int P = 2 + a.n_ls;
    double* __restrict__ x = a.rec + (size_t)r * bat_opt_record(P);
    double *g = x + P, *d = g + P, *xt = d + P, *gn = xt + P, *hy = gn + P, *H = hy + P, *sc = H + P * P;   // sc: f, step length
    int* __restrict__ cn = a.cnt + (size_t)r * BAT_OPT_CNT;
    const double* __restrict__ bd = a.bounds + (int64_t)r * a.bounds_stride;   // the run's own box, or the shared one (stride 0)
    const double INF = __builtin_huge_val();

    double fn = INF;
    if (ok) {
        fn = -bat_lml(sums, n, a.O);
        bat_grad(sums, c, noise, a.n_ls, gn);              // of the LML; f = -LML
        bool finite = isfinite(fn);
        for (int i = 0; i < P; ++i) { gn[i] = -gn[i]; finite = finite && isfinite(gn[i]); }
        if (!finite) fn = INF;
    }
    const int evals = cn[1] + 1;
    cn[1] = evals;
    int iter = cn[0];

    auto finish = [&](const int status) {
        if (status != GPT_OPT_NOT_PD_START)
            for (int i = 0; i < P; ++i) a.theta[(size_t)r * P + i] = x[i];
        a.lml[r] = status != GPT_OPT_NOT_PD_START ? -sc[0] : -INF;
        a.iters[r] = iter;
        a.evals[r] = evals;
        a.status[r] = status;
        return false;
    };
    auto identity = [&] {
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) H[i * P + j] = i == j ? 1.0 : 0.0;
    };

    if (evals == 1) {                                      // the start point
        if (!(fn < INF)) return finish(GPT_OPT_NOT_PD_START);
        for (int i = 0; i < P; ++i) { x[i] = th[i]; g[i] = gn[i]; }
        identity();
        sc[0] = fn;
        cn[0] = iter = 0;
    } else {                                               // a trial point of the line search
        const double f = sc[0];
        double gs = 0.0;
        for (int i = 0; i < P; ++i) gs += g[i] * (th[i] - x[i]);
        if (!(fn < INF && fn <= f + 1e-4 * gs)) {
            const int halvings = cn[2] + 1;
            const double t = 0.5 * sc[1];
            cn[2] = halvings;
            sc[1] = t;
            if (halvings > a.max_ls) return finish(GPT_OPT_LINESEARCH);
            if (evals >= a.max_evals) return finish(GPT_OPT_MAX_EVALS);
            for (int i = 0; i < P; ++i) th[i] = xt[i] = clip(x[i] + t * d[i], bd[2 * i], bd[2 * i + 1]);
            return true;
        }
        double sy = 0.0, ss = 0.0, yy = 0.0;               // accepted: s into d, y into g
        for (int i = 0; i < P; ++i) {
            const double s = th[i] - x[i], y = bd[2 * i] == bd[2 * i + 1] ? 0.0 : gn[i] - g[i];
            d[i] = s;
            g[i] = y;
            sy += s * y; ss += s * s; yy += y * y;
        }
        if (sy > 1e-10 * sqrt(ss * yy)) {                  // H += ((1 + rho y.Hy) rho) s s^T - rho (Hy s^T + s Hy^T)
            const double rho = 1.0 / sy;
            double yHy = 0.0;
            for (int i = 0; i < P; ++i) {
                double h = 0.0;
                for (int j = 0; j < P; ++j) h += H[i * P + j] * g[j];
                hy[i] = h;
                yHy += g[i] * h;
            }
            const double k = (1.0 + rho * yHy) * rho;
            for (int i = 0; i < P; ++i)
                for (int j = 0; j < P; ++j) H[i * P + j] += k * d[i] * d[j] - rho * (hy[i] * d[j] + d[i] * hy[j]);
        }
        for (int i = 0; i < P; ++i) { x[i] = th[i]; g[i] = gn[i]; }
        sc[0] = fn;
        cn[0] = ++iter;
        if (f - fn <= a.ftol * fmax(fmax(fabs(f), fabs(fn)), 1.0)) return finish(GPT_OPT_FTOL);
    }

    // the next iteration: stopping tests, active set, direction, first trial point
    double pgmax = 0.0;
    unsigned active = 0;
    for (int i = 0; i < P; ++i) {
        const double lo = bd[2 * i], hi = bd[2 * i + 1], xi = x[i], gi = g[i];
        pgmax = fmax(pgmax, fabs(xi - clip(xi - gi, lo, hi)));
        if (lo == hi || (xi <= lo && gi > 0.0) || (xi >= hi && gi < 0.0)) active |= 1u << i;
    }
    if (pgmax <= a.pgtol) return finish(GPT_OPT_PGTOL);
    if (iter >= a.max_iter) return finish(GPT_OPT_MAX_ITER);
    if (evals >= a.max_evals) return finish(GPT_OPT_MAX_EVALS);
    double gd = 0.0;
    for (int i = 0; i < P; ++i) {
        double s = 0.0;
        if (!(active >> i & 1))
            for (int j = 0; j < P; ++j)
                if (!(active >> j & 1)) s += H[i * P + j] * g[j];
        d[i] = -s;
        gd += d[i] * g[i];
    }
    if (!(gd < 0.0)) {
        identity();
        for (int i = 0; i < P; ++i) d[i] = active >> i & 1 ? 0.0 : -g[i];
    }
    double t = 1.0;
    if (iter == 0) {
        double dd = 0.0;
        for (int i = 0; i < P; ++i) dd += d[i] * d[i];
        t = fmin(1.0, 1.0 / sqrt(dd));
    }
    sc[1] = t;
    cn[2] = 0;
    for (int i = 0; i < P; ++i) th[i] = xt[i] = clip(x[i] + t * d[i], bd[2 * i], bd[2 * i + 1]);
    return true;
}

template <int NMAX, int KT>
__global__ __launch_bounds__(BatCfg<NMAX>::NT) void bat_optimize(BatOptArgs a) {
    using Cfg = BatCfg<NMAX>;
    constexpr int NT = Cfg::NT, LD = Cfg::LD;
    extern __shared__ __attribute__((aligned(16))) double bat_lds[];
    double* __restrict__ A = bat_lds;                    // NMAX x LD
    double* __restrict__ buf = A + NMAX * LD;            // n x O
    double* __restrict__ dinv = buf + NMAX * BAT_MAX_O;  // 1 / L_ii
    __shared__ double red[BAT_RED][NT / 64];
    __shared__ double th[BAT_OPT_MAX_P];                 // the pending trial point
    __shared__ int go;

    const int r = a.list[blockIdx.x], b = a.run_model[r], tid = threadIdx.x;
    const int64_t n0 = a.n_begin[b];
    const int n = (int)(a.n_begin[b + 1] - n0);
    const int D = a.D, P = 2 + a.n_ls;
    BatArgs fa{};                                        // what bat_factor_body reads of bat_factor's arguments
    fa.X = a.X; fa.Y = a.Y; fa.D = D; fa.O = a.O; fa.n_ls = a.n_ls; fa.jitter = a.jitter;

    if (tid == 0) {                                      // before its first evaluation a run's start waits in theta, later in the record
        const double* __restrict__ src = a.cnt[(size_t)r * BAT_OPT_CNT + 1] == 0 ? a.theta + (size_t)r * P
                                                                                  : a.rec + (size_t)r * bat_opt_record(P) + 3 * P;
        for (int i = 0; i < P; ++i) th[i] = src[i];
    }
    __syncthreads();
    for (int e = 0; e < a.evals_per_launch; ++e) {
        const double c = exp(th[0]), noise = exp(th[1 + a.n_ls]);
        double il[MAX_DIMS];
#pragma unroll
        for (int k = 0; k < MAX_DIMS; ++k) il[k] = k < D ? 1.0 / exp(th[1 + (a.n_ls == 1 ? 0 : k)]) : 0.0;
        double sums[BAT_RED];                            // zeroed by the body
        // th is not written before every thread has passed the body's first barrier, go not before the barrier below
        const bool ok = bat_factor_body<NMAX, KT, true>(fa, b, n0, n, c, noise, il, A, buf, dinv, red, sums);
        if (tid == 0) go = opt_advance(a, r, n, ok, sums, c, noise, th);
        __syncthreads();
        if (!go) break;                                  // the same LDS value in every thread
    }
}

template <int NMAX>
void launch_optimize(int ktype, int count, hipStream_t s, const BatOptArgs& a) {
    using Cfg = BatCfg<NMAX>;
    if (count < 1) return;
    with_kernel_type(ktype, [&](auto kt) {
        constexpr int KT = decltype(kt)::value;
        if constexpr (NMAX > BAT_SMALL_N) launch_lds<bat_optimize<NMAX, KT>>(dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
        else hipLaunchKernelGGL((bat_optimize<NMAX, KT>), dim3(count), dim3(Cfg::NT), Cfg::factor_lds, s, a);
    });
}

}  // namespace

void launch_bat_optimize(hipStream_t s, int ktype, int n_small, int n_large, const BatOptArgs& a) {
    launch_optimize<BAT_SMALL_N>(ktype, n_small, s, a);
    BatOptArgs large = a;
    large.list += n_small;
    launch_optimize<BAT_MAX_N>(ktype, n_large, s, large);
}

}  // namespace gpt
