// coop_kernel.h -- the kernels that are instantiated per distribution kind: norm_kernel<KIND>, coop_kernel<P> with its two
// problems (SymphonyProblem<KIND>, HeyvaertsProblem<KIND>) and the two unit seams gamma_integral_kernel<KIND> and
// integrand_kernel_n<KIND>.  rimphony_hip.hip instantiates them for the four analytic distributions, rimphony_tab.hip for
// the tabulated one: separate translation units, because hipcc's code generation for one big kernel depends on what else
// is in the unit (rimphony_internal.h) -- a fifth kind must not move the other four.  (group_kernel.h is the same split for
// group_kernel<P>: rimphony_group.hip and rimphony_tab_group.hip.)
#ifndef RIM_COOP_KERNEL_H
#define RIM_COOP_KERNEL_H

#include <hip/hip_runtime.h>
#include "symphony_wave.h"
#include "heyvaerts_wave.h"
#include "rimphony_internal.h"
#include "coop_common.h"

// ------------------------------------------------------------------------------
// normalisation integrands (power_law.rs:95-96, pitchy_kappa.rs:100-104; the
// thermal one is the substituted form documented in oracle/rimo_dist.c)
// ------------------------------------------------------------------------------

template <int KIND>
__device__ inline double norm_integrand(const DistParams &d, double g)
{
    if (KIND == DIST_POWER_LAW || KIND == DIST_PITCHY_PL) {
        return rim_pow(g, -d.par[0]) * rim_exp(-g * d.inv_gamma_cutoff);
    } else if (KIND == DIST_PITCHY_KAPPA) {
        return g * rim_sqrt(g * g - 1.) *
            rim_pow(1. + (g - 1.) * d.inv_kappa_width, -(d.par[0] + 1.)) *
            rim_exp(-g * d.inv_gamma_cutoff);
    } else {
        const double u = g;
        const double u2 = u * u;
        const double gg = 1. + u2;
        return gg * (u * rim_sqrt(u2 + 2.)) * rim_exp(d.neg_inverse_t * gg) * (2. * u);
    }
}

__device__ inline double hyperg_2F1_at_1(double a, double b, double c)
{
    const double lc = rim_lgamma_pos(c);
    const double lcab = rim_lgamma_pos(c - a - b);
    const double lca = rim_lgamma_pos(c - a);
    const double lcb = rim_lgamma_pos(c - b);
    return rim_exp(lc + lcab - lca - lcb);
}

// nbar(gamma) of a row of a family of 2-D surfaces (dev_symphony.h: tab_2d_norm_integrand on the row's line).  Defined by the
// units of those forms, next to the Kronrod tables it reads (tab_2d_family_unit.h); no other instantiation of norm_kernel names it.
template <int KIND>
__device__ double tab_2d_family_nbar(const DistParams &d, double g);

template <int KIND>
__global__ __launch_bounds__(64) void norm_kernel(ParamPtrs pp, size_t n, double *norm, unsigned long long *queue,
                                                    double *spill_base)
{
    __shared__ double s_tab[96];
    __shared__ double s_store[RIM_ISTORE_DOUBLES(CAP_NORM)];
    const GKLane g = gk_lane_init(s_tab);
    const IStore st = istore_carve(s_store, CAP_NORM, spill_base + (size_t) blockIdx.x * SPILL_DOUBLES_PER_WAVE, SPILL_INNER);
    __shared__ QagPark s_qpark;
    if (threadIdx.x == 0) { s_qpark.ctr = WaveCounters{0, 0, 0}; s_qpark.hb = nullptr; }

    for (;;) {
        const unsigned long long t = wave_next_task(queue, g.lane);
        if (t >= n) break;
        const size_t i = (size_t) t;

        DistParams d;
        load_params<KIND>(pp, i, d);
        // (the tabulated kind: dist_prepare replaces the table index in par[0], so the index is judged first)
        constexpr bool TAB = KIND == DIST_TABULATED || KIND == DIST_TABULATED_PITCHY || KIND == DIST_TABULATED_GRID || tab_kind_family(KIND) ||
            tab_kind_2d_family(KIND);
        // (a family judges a real index: x in [0, n_tables - 1])
        size_t fam_a;
        double fam_w;
        bool tab_ok = !TAB || (tab_kind_family(KIND) || tab_kind_2d_family(KIND) ? tab_family_row(pp.p[1], d.par[0], fam_a, fam_w)
                                                                                 : tab_row_ok(pp.p[1], d.par[0]));
        // (a cubic blend of the tables' k may leave [0, 100] between two knots: such a row names no distribution either)
        if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY)
            tab_ok = tab_ok && tab_2d_family_cubic_k_ok((const double *) (uintptr_t) rim_bits(d.par[2]));
        dist_prepare<KIND>(d, RIM_NAN);

        double lo, hi, epsrel, pa = 1.;
        if (TAB) {
            // (a row whose index names no table: NaN, and with it RIMPHONY_ST_NORM_FAIL in every selected slot)
            if (!tab_ok) { if (g.lane == 0) norm[i] = RIM_NAN; continue; }
            lo = d.inv_kappa_width; hi = d.neg_inverse_t; epsrel = 1e-8;
            // a pitch row: P = 1/2 int g dmu of its header takes the place of the pitchy kinds' 2F1 (pitchy_pl.rs:98-111)
            // (a sin^k set: every table has one, with the factor in it -- NaN where its quadrature failed)
            if (tab_norm_has_pitch<KIND>(d)) pa = ((const double *) (uintptr_t) rim_bits(d.par[0]))[TAB_PITCH_P];
        } else if (KIND == DIST_POWER_LAW) { lo = d.par[1]; hi = d.par[2]; epsrel = 1e-8; }
        else if (KIND == DIST_PITCHY_PL) { lo = d.par[2]; hi = d.par[3]; epsrel = 1e-8; pa = hyperg_2F1_at_1(0.5, -0.5 * d.par[1], 1.5); }
        else if (KIND == DIST_PITCHY_KAPPA) {
            const double g_cut = 1. / d.inv_gamma_cutoff;
            lo = 1.; hi = 1e3 * g_cut; epsrel = 1e-8; pa = hyperg_2F1_at_1(0.5, -0.5 * d.par[2], 1.5);
        } else { lo = 0.; hi = rim_sqrt(60. * d.par[0] + 4.); epsrel = 1e-10; }

        // (the tabulated kind's integrand, n(gamma) of its table, is dev_symphony.h's: the tests' table oracle shares it)
        // (a family of 2-D surfaces: nbar of the row's blended surface, the quadrature the plain 2-D forms run per table at install)
        auto f = [&](double x, bool active) -> double {
            if constexpr (tab_kind_2d_family(KIND)) return active ? tab_2d_family_nbar<KIND>(d, x) : 0.;
            if (TAB) return active ? tab_norm_integrand<KIND>(d, x) : 0.;
            return active ? norm_integrand<KIND>(d, x) : 0.;
        };
        QagState q;
        wave_qag(f, g, st, lo, hi, 0., epsrel, 1000, q, &s_qpark);
        double v = RIM_NAN;
        if (q.status == QAG_SUCCESS) {
            if (KIND == DIST_PITCHY_PL || KIND == DIST_PITCHY_KAPPA || (TAB && tab_norm_has_pitch<KIND>(d)))
                v = 1. / (2. * RIM_TWO_PI * pa * q.result);
            else v = 1. / (2. * RIM_TWO_PI * q.result);
        }
        if (g.lane == 0) norm[i] = v;
    }
}

// ------------------------------------------------------------------------------
// symphony
// ------------------------------------------------------------------------------

#if defined(RIM_PROF)
#define RIM_PROF_ROWS 32768
static __device__ unsigned long long g_rim_prof[RIM_PROF_ROWS * 32];     // (one per translation unit)
#endif

// ---- the two problems the cooperative kernel runs ------------------------------------------
// A problem supplies the uniform context of a task, the parked task state and the five steps of
// the resumable computation (begin / post / eval / consume / result).  Requests and results have
// the same shape in both: (double abscissa, int tag) -> (double value, int status).
template <int KIND, int PREC = 0>
struct SymphonyProblem {
    struct Ctx { SymPoint pt; DistParams d; };
    typedef TaskState Task;
    typedef QagPark Park;
    enum : unsigned long long { QUEUE = 0, WAVES = RIM_SYM_WAVES, HB_TAG = 0, EXTRA_LDS_DOUBLES = 1, EARLY_HELP = 0, EARLY_SQUAD = 0 };
    static __device__ __forceinline__ void init(const SymArgs &, Ctx &, double *) {}
    static __device__ __forceinline__ void load(const SymArgs &a, size_t i, int slot, Ctx &c, double &norm)
    { load_context<KIND>(a, i, slot, c.pt, c.d, norm); }
    static __device__ __forceinline__ void begin(const Ctx &c, Task &T) { sym_begin(c.pt, T); }
    static __device__ __forceinline__ int early_metric(const Task &) { return 0; }
    static __device__ __forceinline__ void uniformize(Task &T) { task_uniformize(T); }
    static __device__ __forceinline__ bool done(const Task &T) { return T.phase == PH_DONE; }
    struct Stash { unsigned used; };        // (rounds are the Faraday kernel's: HeyvaertsProblem)
    enum { TURBO = 0 };
    static __device__ __forceinline__ void post(const Ctx &c, const GKLane &g, const IStore &outer, Task &T, SymBatch &B, Stash *, int)
    { sym_post(c.pt, g, outer, T, B); }
    static __device__ __forceinline__ int round_n(const Stash &) { return 1; }
    static __device__ __forceinline__ void round_drop(Stash &) {}
    static __device__ __forceinline__ double round_request(const Stash &, const GKLane &, int) { return 0.; }

    // one or two requests ((x1, tag1) only if have1): two gamma-integrals share their first rule application
    static __device__ __forceinline__ void eval2(const Ctx &c, const GKLane &g, const IStore &inner, Park *qp,
                                                 double x0, int tag0, double x1, int tag1, bool have1,
                                                 double &v0, int &st0, double &v1, int &st1)
    { sym_eval_pair<KIND, PREC>(c.pt, c.d, g, inner, qp, x0, tag0, x1, tag1, have1, v0, st0, v1, st1); }
    static __device__ __forceinline__ void consume(const Ctx &c, const GKLane &g, const IStore &outer, Task &T,
                                                   const SymBatch &B, double gval, int bst, Stash *, unsigned long long *, unsigned long long *,
                                                   const AssistSlot *, int, int)
    { sym_consume(c.pt, g, outer, T, B, gval, bst); }
    static __device__ __forceinline__ double result(const Ctx &c, const Task &T, int &st) { return sym_result(c.pt, T, st); }
};

template <int KIND>
struct HeyvaertsProblem {
    struct Ctx { HeyPoint pt; DistParams d; HeyConsts hc; };
    typedef HeyTask Task;
    typedef QagParkBase Park;
    // EARLY_SQUAD: the default size of the squad that serves the longest outer quadrature from the start of a launch
    // (coop_common.h).  Outer quadratures that run to GSL's limit of 4096 bisections occur on the power-law table (one
    // task in ~1e5: 4122 / 3775 batches -- one title, 64 waves) and on the pitchy-kappa table (four of 2844 .. 4132
    // batches among the first 16793 rows and a dozen of 300 .. 760 -- four titles, 256 waves); the thermal table's long
    // chains were the endless marching loops that hey_qr_is_endless() now ends at once, the pitchy power-law table has
    // none past 244 batches -- there the squad would only cost its share of the grid.
    enum : unsigned long long { QUEUE = 4, WAVES = RIM_HEY_WAVES, HB_TAG = 1ull << 62, EXTRA_LDS_DOUBLES = 1, EARLY_HELP = 1,
                                EARLY_SQUAD = KIND == DIST_POWER_LAW ? RIM_EARLY_SQUAD_DEFAULT : KIND == DIST_PITCHY_KAPPA ? 4 * RIM_EARLY_SQUAD_DEFAULT : 0 };
    static __device__ __forceinline__ void init(const SymArgs &a, Ctx &c, double *extra_lds)
    {
        c.hc = hey_consts();
    }
    static __device__ __forceinline__ void load(const SymArgs &a, size_t i, int slot, Ctx &c, double &norm)
    {
        HeyPoint &pt = c.pt;
        pt.s = uni(a.s[i]);
        rim_sincos(a.theta[i], &pt.sin_th, &pt.cos_th);
        pt.sin_th = uni(pt.sin_th);
        pt.cos_th = uni(pt.cos_th);
        hey_point_derive(pt);
        pt.sigma0 = uni(pt.sigma0); pt.sigma0_sq = uni(pt.sigma0_sq); pt.dinv = uni(pt.dinv);
        pt.stokes = uni(c_slot_stokes[slot]);
        load_params<KIND>(a.pp, i, c.d);
        norm = uni(a.norm[i]);
        dist_prepare<KIND>(c.d, norm);
#pragma unroll
        for (int k = 0; k < 5; k++) c.d.par[k] = uni(c.d.par[k]);
        c.d.inv_gamma_cutoff = uni(c.d.inv_gamma_cutoff);
        c.d.inv_kappa_width = uni(c.d.inv_kappa_width);
        c.d.neg_inverse_t = uni(c.d.neg_inverse_t);
        hey_point_endless<KIND>(pt, c.d);
        pt.endless_gamma = uni(pt.endless_gamma);
    }
    static __device__ __forceinline__ void begin(const Ctx &c, Task &T) { hey_begin(c.pt, T); }
    // what a task competes for early help with: the subintervals of the outer quadrature in progress (0 outside one).
    // A quadrature that converges stays below a few dozen; one on its way to GSL's limit of 4096 (heyvaerts.rs:82-83)
    // adds one per batch, for thousands of batches.
    static __device__ __forceinline__ int early_metric(const Task &T)
    { return (T.phase == HP_QAG_BISECT || T.phase == HP_QAG_FIRST) ? T.oq.size : 0; }
    static __device__ __forceinline__ void uniformize(Task &T) { hey_uniformize(T); }
    static __device__ __forceinline__ bool done(const Task &T) { return T.stage == HS_DONE; }
    typedef HeyStash Stash;
    // rounds (heyvaerts_wave.h): a long outer quadrature's batch carries the children of up to RIM_TURBO_MAX intervals.
    // Compiled in for the pitchy-kappa distribution only: that is where they pay (four quadratures of 2844 .. 4132 batches
    // and a dozen of 300 .. 760 in 65536 rows: -20 .. -26 % on its Faraday launches); the power-law table's long
    // quadratures are hidden by the squad already, the other two tables have none -- and the code costs a kernel that
    // never sees a round about 1 % (profiles/r4_ab_rounds.txt).
    enum { TURBO = KIND == DIST_PITCHY_KAPPA ? 1 : 0 };
    static __device__ __forceinline__ void post(const Ctx &c, const GKLane &g, const IStore &outer, Task &T, SymBatch &B, Stash *hs, int rounds)
    { hey_post(c.pt, g, outer, T, B, hs, rounds); }
    static __device__ __forceinline__ int round_n(const Stash &hs) { return uni(hs.round_n); }
    static __device__ __forceinline__ void round_drop(Stash &hs) { hs.round_n = 1; hs.hit = -1; }
    static __device__ __forceinline__ double round_request(const Stash &hs, const GKLane &g, int j) { return hey_round_request(&hs, g, j); }
    // file the sums of the round's further intervals: lane `rank`-th request of interval j sits at 62 j + rank of the slot
    static __device__ __forceinline__ void eval2(const Ctx &c, const GKLane &g, const IStore &inner, Park *qp,
                                                 double x0, int tag0, double x1, int tag1, bool have1,
                                                 double &v0, int &st0, double &v1, int &st1)
    { hey_eval_pair<KIND>(c.pt, c.d, c.hc, g, inner, qp, x0, tag0, x1, tag1, have1, v0, st0, v1, st1); }
    static __device__ __forceinline__ void consume(const Ctx &c, const GKLane &g, const IStore &outer, Task &T,
                                                   const SymBatch &B, double gval, int bst, Stash *hs, unsigned long long *stash_samples,
                                                   unsigned long long *dropped_samples, const AssistSlot *slot, int rank, int per)
    {
        // (a round's further intervals: their values, status bits and sample counts are read from the owner's board slot)
        HeyRoundIO io;
        io.res = slot->res; io.res_status = slot->res_status; io.res_samples = slot->res_samples; io.rank = rank; io.per = per;
        hey_consume(c.pt, g, outer, T, B, gval, bst, hs, stash_samples, dropped_samples, &io);
    }
    static __device__ __forceinline__ double result(const Ctx &, const Task &T, int &st) { return hey_result(T, st); }
};

template <class P>
__global__ __launch_bounds__(64, P::WAVES) void coop_kernel(SymArgs a)
{
#if defined(RIM_PROF) && defined(__HIP_DEVICE_COMPILE__)
    if (threadIdx.x < 32) rim_prof_lds[threadIdx.x] = 0;
    __syncthreads();
#endif
    RIM_PROF_T(t_kernel);
    __shared__ double s_tab[96];
    __shared__ double s_inner[RIM_ISTORE_DOUBLES(CAP_INNER)];
    __shared__ double s_outer[RIM_ISTORE_DOUBLES(CAP_OUTER)];
    __shared__ typename P::Task s_park;
    const GKLane g = gk_lane_init(s_tab);
    const int lane = g.lane;
    double *spill = a.spill + (size_t) blockIdx.x * SPILL_DOUBLES_PER_WAVE;
    const IStore inner = istore_carve(s_inner, CAP_INNER, spill, SPILL_INNER);
    const IStore outer = istore_carve(s_outer, CAP_OUTER, spill + RIM_ISTORE_DOUBLES(SPILL_INNER), SPILL_OUTER);
    __shared__ typename P::Park s_qpark;
    __shared__ double s_extra[P::EXTRA_LDS_DOUBLES];
    __shared__ typename P::Stash s_stash;       // rounds of a long outer quadrature (Faraday kernel; heyvaerts_wave.h)
    if (threadIdx.x == 0) { s_qpark.ctr = WaveCounters{0, 0, 0}; s_qpark.hb = nullptr; s_stash.used = 0; P::round_drop(s_stash); }
    bool last_shared = false;                   // the previous batch of the own task went over the board: the next may carry a round
    int round_n = 1;                            // intervals whose children the current batch evaluates

    AssistSlot *const my = a.board + blockIdx.x;
    unsigned *const flag_exhausted = a.board_flags + BOARD_FLAG_EXHAUSTED;
    unsigned *const flag_active = a.board_flags + BOARD_FLAG_ACTIVE;
    unsigned *const flag_idle = a.board_flags + BOARD_FLAG_IDLE;
    unsigned *const hints = a.board_flags + BOARD_HINTS;
    const unsigned nboard = gridDim.x;
    unsigned seq = 0;                      // sequence number of this wave's published batches
    bool counted_idle = false;             // this wave is currently counted in flags[IDLE]
    int backoff = 1;
    unsigned long long idle_since = 0;     // wall clock of the first empty poll since this wave last evaluated a request
    // diagnostics of the cooperative tail (queue words 8..13)
    unsigned n_polls = 0;
#if defined(RIM_COOP_DIAG)
    unsigned long long n_shared_batches = 0, n_helper_reqs = 0, n_owner_shared_reqs = 0, wait_ticks = 0,
                       n_empty_claims = 0, eval_ticks = 0, max_wait = 0, n_polls_total = 0;
#define COOP_DIAG(x) x
#else
#define COOP_DIAG(x)
#endif

    const unsigned long long ntasks = (unsigned long long) a.n * (unsigned long long) a.nslots;
    typename P::Ctx cx;                    // context of the requests being evaluated (own task or a helped one)
    P::init(a, cx, s_extra);
    unsigned long long *const queue = a.queue + P::QUEUE;
    // The own task's state lives in LDS (s_park) between the three places that touch it, so that it
    // never occupies registers while the integrand runs.
    size_t own_i = 0;
    int own_slot = 0;
    bool have_task = false, helper = false;
    bool board_dead = false;               // this wave once gave up waiting for helpers: it never publishes again (below)
    unsigned last_hint = 0;                // lane 0: the hint whose batch this wave has already seen exhausted

    // early help for the launch's longest chain (coop_common.h, SymArgs::early_squad)
    // (early_classes titles, each with its own 64 waves of the squad -- the ones that listen to the hint lines l with
    // l & (classes - 1) == title.  A task competes for one title at a time, starting with block & (classes - 1); when a
    // longer quadrature holds that one it moves to the title with the shortest holder, so that the titles end up with
    // the `classes` longest quadratures in progress and that many chains are served side by side.  Measured and not kept:
    // every champion publishing to the whole squad, eight titles on 256 waves -- the hint traffic slowed the bulk.)
    unsigned title = (unsigned) blockIdx.x & (a.early_classes - 1u);
    unsigned *const flag_champ0 = a.board_flags + BOARD_FLAG_CHAMP;
    const bool early_on = P::EARLY_HELP && a.early_squad != 0u && a.board != nullptr;
    const bool squad = early_on && (unsigned) blockIdx.x % a.early_stride == 0u && (unsigned) blockIdx.x / a.early_stride < a.early_squad;
    unsigned champ_mine = 0;               // the word this wave last entered in flags[CHAMP] (0: none)
    bool champion = false;                 // ... and it was the maximum: this task publishes while the queue is full
    bool seen_exhausted = false;           // (squad) the queue has run dry: from here on an ordinary helper of the tail
#if defined(RIM_TAIL_DIAG)
    unsigned long long task_t0 = 0;
    unsigned n_champ_batches = 0;
#endif

    // issue priorities: 3 the champion and the squad that serves it (the chain is the launch's critical path), 2 every
    // other owner, 0 the helpers of the tail
    __builtin_amdgcn_s_setprio(2);
    for (;;) {
        SymBatch B;
        B.req_n = 0.; B.req_lobe = 0; B.req_active = false; B.n_req = 0; B.phase = PH_DONE;
        AssistSlot *src = my;
        unsigned src_seq = 0;
        unsigned long long mask = 0;
        bool shared = false;

        if (!helper) {
            // ---------- owner: next batch of the current task (fetching a task first if needed) ----------
            if (!have_task) {
                // (a wave of the squad never fetches a task: it becomes a helper right here, without touching the queue --
                // the host left it out of flags[ACTIVE])
                const unsigned long long t = squad ? ~0ull : wave_next_task(queue, lane);
                if (t >= ntasks) {
                    helper = true;
                    if (lane == 0) {
                        if (!squad) {
#if defined(RIM_TAIL_DIAG)     // (tools/tail_times.py: when did the queue run dry, when did the launch end)
                            atomicCAS(a.queue + (P::QUEUE ? 10 : 12), 0ull, wall_clock64());
#endif
                            __hip_atomic_store(flag_exhausted, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_fetch_sub(flag_active, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        if (a.board) __hip_atomic_fetch_add(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    counted_idle = true;      // flags[IDLE] = helper waves that are not evaluating a request
                    // Helpers run below the issue priority of waves that own a task: an owner's serial
                    // bookkeeping between batches is the critical path of the tail.  (The squad keeps the champion's
                    // priority until the queue is dry.)
                    if (squad) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(0);
                    if (!a.board) break;     // cooperation disabled
                    continue;
                }
                const size_t seqidx = (size_t) (t / (unsigned) a.nslots);
                own_i = a.perm ? (size_t) a.perm[seqidx] : seqidx;
                own_slot = a.slot[(int) (t % (unsigned) a.nslots)];
                double norm;
                P::load(a, own_i, own_slot, cx, norm);
                if (lane == 0) {
                    s_qpark.hb = (a.heartbeat && (t | (unsigned long long) P::HB_TAG) == a.hb_task) ? a.heartbeat : nullptr;
                    if (s_qpark.hb) hb_store(s_qpark.hb + 0, t + 1);
                }
                __syncthreads();
                if (!(norm == norm)) {
                    if (lane == 0) {
                        a.out[own_i * 8 + own_slot] = RIM_NAN;
                        if (a.status) a.status[own_i * 8 + own_slot] = ST_NORM_FAIL | ST_NONFINITE;
                    }
                    continue;
                }
                typename P::Task T0;
                P::begin(cx, T0);
                if (lane == 0) { s_park = T0; s_stash.used = 0; }
                __syncthreads();
                have_task = true;
                last_shared = false;
#if defined(RIM_TAIL_DIAG)
                task_t0 = wall_clock64();
#endif
            }
            bool finished;
            int task_batches = 0;            // (the task's early-help metric after this post)
            {
                typename P::Task T = s_park;
                P::uniformize(T);
                if (!P::done(T)) P::post(cx, g, outer, T, B, P::TURBO ? &s_stash : nullptr, (P::TURBO && a.turbo && last_shared && !board_dead) ? RIM_TURBO_MAX - 1 : 0);
                finished = P::done(T);
                task_batches = P::early_metric(T);
                round_n = P::TURBO ? P::round_n(s_stash) : 1;
                if (finished) {
                    int st = 0;
                    const double val = P::result(cx, T, st);
                    // the heaviest task of the launch: its sequential chain of batches bounds the launch's tail
                    // (queue word 15 of the kernel's block: (batches << 40) | point index; rimphony_last_tail)
                    if (lane == 0) atomicMax(a.queue + (P::QUEUE ? 15 : 14), ((unsigned long long) T.batches << 40) | ((unsigned long long) own_i & 0xffffffffffull));
                    if (lane == 0) {
                        a.out[own_i * 8 + own_slot] = val;
#if defined(RIM_TAIL_DIAG)     // (tools/tail_times.py: when a chain of >= 512 batches began and ended -- the last one to end is reported)
                        if (P::QUEUE && T.batches >= 2048) { a.queue[8] = task_t0; a.queue[9] = wall_clock64(); a.queue[14] = n_champ_batches; }
                        n_champ_batches = 0;
#endif
#if defined(RIM_TAIL_DIAG)     // (tools/tail_times.py: the task's number of batches in the upper half of the status word)
                        if (a.status) a.status[own_i * 8 + own_slot] = st | ((T.batches < 0x7fff ? T.batches : 0x7fff) << 16);
#else
                        if (a.status) a.status[own_i * 8 + own_slot] = st;
#endif
                        if (s_qpark.hb) hb_store(s_qpark.hb + 10, 1ull);
                    }
                } else {
                    __syncthreads();              // everyone has read s_park
                    if (lane == 0) s_park = T;    // state after posting (batch counter, picked interval)
                }
            }
            if (finished) {
                if (champ_mine) {
                    // give the title back (if it is still this task's): the other candidates enter again with their next batch
                    if (lane == 0) {
                        unsigned expect = champ_mine;
                        __hip_atomic_compare_exchange_strong(flag_champ0 + 32u * title, &expect, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
                    }
                    champ_mine = 0;
                    if (champion) __builtin_amdgcn_s_setprio(2);
                    champion = false;
                }
                have_task = false;
                continue;
            }
            mask = wv_ballot(B.req_active);

            // publish the batch when some wave is idle -- or, while the queue is still full, when this task holds the
            // most batches of all tasks in flight (the squad serves it)
            unsigned idle = 0, act = 1, exhausted = 0, champ_now = 0, title_next = title;
            const unsigned cand = (early_on && !board_dead && task_batches >= a.early_min)
                ? (((unsigned) (task_batches < 0xffff ? task_batches : 0xffff) << 16) | ((unsigned) blockIdx.x + 1u)) : 0u;
            if (lane == 0 && a.board) {
                exhausted = __hip_atomic_load(flag_exhausted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (exhausted) {
                    idle = __hip_atomic_load(flag_idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    act = __hip_atomic_load(flag_active, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (cand | champ_mine) {
                    if (cand < champ_mine) {
                        // the quadrature that competed for the title is over: give it back if it is still this task's
                        unsigned expect = champ_mine;
                        __hip_atomic_compare_exchange_strong(flag_champ0 + 32u * title, &expect, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (cand) {
                        champ_now = __hip_atomic_load(flag_champ0 + 32u * title, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (champ_now > cand) {
                            // a longer quadrature holds this title (this task's own entry, if any, is gone with it): compete
                            // for the title whose holder is the shortest
                            for (unsigned k = 0; k < a.early_classes; k++) {
                                const unsigned v = __hip_atomic_load(flag_champ0 + 32u * k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (v < champ_now) { champ_now = v; title_next = k; }
                            }
                        }
                        if (champ_now < cand) {
                            const unsigned old = __hip_atomic_fetch_max(flag_champ0 + 32u * title_next, cand, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT);
                            champ_now = old > cand ? old : cand;
                        }
                    }
                }
            }
            title = (unsigned) __builtin_amdgcn_readfirstlane((int) title_next);
            idle = (unsigned) __builtin_amdgcn_readfirstlane((int) idle);
            act = (unsigned) __builtin_amdgcn_readfirstlane((int) act);
            exhausted = (unsigned) __builtin_amdgcn_readfirstlane((int) exhausted);
            champ_now = (unsigned) __builtin_amdgcn_readfirstlane((int) champ_now);
            if (early_on) {
                champ_mine = cand;
                const bool is_champ = cand != 0u && !exhausted && champ_now == cand;
                if (is_champ != champion) { if (is_champ) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2); }
                champion = is_champ;
            }
            const int cnt = __builtin_popcountll(mask);
            shared = (exhausted ? idle != 0 : champion) && cnt >= 2 && !board_dead;
            if (P::TURBO) {
                if (cnt != 0) last_shared = shared;     // (a bisection booked from the stash posts nothing and changes nothing)
                if (round_n > 1 && !shared) {
                    // the round was planned for a batch that does not go over the board after all: the picked interval only
                    __syncthreads();
                    if (lane == 0) P::round_drop(s_stash);
                    __syncthreads();
                    round_n = 1;
                }
            }
#if defined(RIM_TAIL_DIAG)     // (tools/tail_times.py: when the longest outer quadrature passed 64 / 512 / 2048 subintervals, and how
                               // many of its batches were published as the champion's)
            if (P::QUEUE && lane == 0) {
                if (task_batches == 64) atomicCAS(a.queue + 12, 0ull, wall_clock64());
                if (task_batches == 512) atomicCAS(a.queue + 13, 0ull, wall_clock64());
                if (task_batches == 2048) a.queue[2] = wall_clock64();
            }
            if (shared && !exhausted) n_champ_batches += 1;
#endif
            if (shared) {
                seq += 1;
                src_seq = seq;
                COOP_DIAG(n_shared_batches += 1;)
                if (P::TURBO && round_n > 1) __syncthreads();      // lane 0's copy of the task state (the round's intervals) is visible
                if (B.req_active) {
                    const int rank = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                    bput(&my->req_n[rank], rim_bits(B.req_n));
                    bput(&my->req_lobe[rank], B.req_lobe);
                    // a round: the children of the further intervals, `cnt` requests each, behind the picked interval's
                    for (int j = 1; j < round_n; j++) {
                        bput(&my->req_n[cnt * j + rank], rim_bits(P::round_request(s_stash, g, j)));
                        bput(&my->req_lobe[cnt * j + rank], B.req_lobe);
                    }
                }
                if (lane == 0) {
                    bput(&my->point, (unsigned long long) own_i);
                    bput(&my->slot, own_slot);
                    bput(&my->done, 0u);
                }
                drain_vmem();
                __syncthreads();
                if (lane == 0)
                    __hip_atomic_store(&my->claim, ((unsigned long long) seq << 32) | ((unsigned long long) (cnt * round_n) << 8),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                drain_vmem();          // the claim word is out before anybody can see the hint
                __syncthreads();
                {
                    // (while the queue is full the only listeners are the squad: every hint line of the title)
                    const unsigned span = exhausted ? hint_span(act) : a.early_classes;
                    const unsigned channel = exhausted ? (((unsigned) blockIdx.x + seq) & (span - 1u)) : title;
                    if (((unsigned) lane & (span - 1u)) == channel)
                        __hip_atomic_store(&hints[(unsigned) lane * BOARD_HINT_STRIDE], (seq << 16) | ((unsigned) blockIdx.x + 1u),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        } else {
            // ---------- helper: find a published batch through this wave's hint line ----------
            unsigned h = 0, act = 1, exh = 0;
            int leave = 0;
            unsigned long long c = 0;
            if (lane == 0) {
                if ((n_polls & 15u) == 0) {
                    act = __hip_atomic_load(flag_active, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (squad && !seen_exhausted) exh = __hip_atomic_load(flag_exhausted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    // More idle waves than the remaining owners can feed (a batch has <= 62 requests) only
                    // add polling traffic, which slows the waves that compute: the surplus leaves.
                    const unsigned keep = act * 64u + 32u;
                    if (counted_idle && act != 0 &&
                        __hip_atomic_load(flag_idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > keep) {
                        const unsigned before = __hip_atomic_fetch_sub(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (before > keep) leave = 1;
                        else __hip_atomic_fetch_add(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (!leave)
                    h = __hip_atomic_load(&hints[((unsigned) blockIdx.x & 63u) * BOARD_HINT_STRIDE], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
                const unsigned hs = h & 0xffffu;
                if (h != last_hint && hs != 0 && hs <= nboard) {
                    c = __hip_atomic_load(&a.board[hs - 1].claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (!claim_open(c)) { last_hint = h; h = 0; }      // nothing left of that batch: wait for a new hint
                } else {
                    h = 0;
                }
            }
            h = (unsigned) __builtin_amdgcn_readfirstlane((int) h);
            act = (unsigned) __builtin_amdgcn_readfirstlane((int) act);
            if (__builtin_amdgcn_readfirstlane(leave)) break;
            if (squad && !seen_exhausted && __builtin_amdgcn_readfirstlane((int) exh)) {
                seen_exhausted = true;
                __builtin_amdgcn_s_setprio(0);
            }
            n_polls += 1;
            COOP_DIAG(n_polls_total += 1;)
            if (h == 0) {
                if (act == 0) break;       // every task is finished
                if (squad && !seen_exhausted) idle_since = 0;      // the squad waits for a champion as long as the queue is full
                // A wave that has seen nothing to do for 2 s leaves.  It holds no claim, so leaving is always safe,
                // and it bounds every wait in this kernel: should part of the grid not be resident (the launch
                // sizes it so that it is), the waves waiting for a slot get one instead of being waited for.
                const unsigned long long now = wall_clock64();
                if (idle_since == 0) idle_since = now;
                else if (now - idle_since > a.idle_ticks) {
                    if (counted_idle && lane == 0)
                        __hip_atomic_fetch_sub(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                for (int w = 0; w < backoff; w++) __builtin_amdgcn_s_sleep(127);
                if (backoff < 16) backoff *= 2;
                continue;
            }
            h &= 0xffffu;
            const unsigned long long cw = bcast_u64(c);
            src = a.board + (h - 1u);
            src_seq = (unsigned) (cw >> 32);
            shared = true;
            // context of the helped task is loaded after the first successful claim (below)
        }

        // ---------- evaluate requests of `src` (the integrand lives here, once) ----------
        int batch_status = 0;
        double gval = 0.;
        bool ctx_loaded = !helper;
        unsigned long long local_mask = mask;
        int got = 0;
        bool redo;
        do {
        redo = false;
        for (;;) {
            int k;
            if (shared) {
                k = assist_claim(src, src_seq, lane);      // ordinal of the request within the batch
            } else {
                k = local_mask ? __builtin_ffsll((long long) local_mask) - 1 : -1;
                local_mask &= local_mask - 1;
            }
            if (k < 0) break;
            got += 1;
            COOP_DIAG(if (shared) { if (helper) n_helper_reqs += 1; else n_owner_shared_reqs += 1; })
            double n;
            int lb;
            if (helper) {
                if (!ctx_loaded) {
                    double norm;
                    const size_t hi = (size_t) bcast_u64(bget(&src->point));
                    const int hs = __builtin_amdgcn_readfirstlane(bget(&src->slot));
                    P::load(a, hi, hs, cx, norm);
                    ctx_loaded = true;
                    if (counted_idle) {
                        if (lane == 0) __hip_atomic_fetch_sub(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        counted_idle = false;
                    }
                    backoff = 1;
                    idle_since = 0;
                }
                n = uni(rim_frombits(bget(&src->req_n[k])));
                lb = __builtin_amdgcn_readfirstlane(bget(&src->req_lobe[k]));
            } else if (P::TURBO && shared && k >= __builtin_popcountll(mask)) {
                // a request of one of the round's further intervals: it only exists on the board
                n = uni(rim_frombits(bget(&my->req_n[k])));
                lb = __builtin_amdgcn_readfirstlane(bget(&my->req_lobe[k]));
            } else {
                const int kl = shared ? kth_set_bit(mask, k) : k;     // lane that posted the request
                n = readlane_d(B.req_n, kl);
                lb = wv_readlane(B.req_lobe, kl);
            }
            // a wave working through its own batch starts two requests together (P::eval2)
            int k2 = -1;
            double n2 = n;
            int lb2 = lb;
            if (!shared && local_mask) {
                k2 = __builtin_ffsll((long long) local_mask) - 1;
                local_mask &= local_mask - 1;
                n2 = readlane_d(B.req_n, k2);
                lb2 = wv_readlane(B.req_lobe, k2);
            }
            if (lane == 0 && s_qpark.hb) {
                hb_store(s_qpark.hb + 8, (unsigned long long) k);
                hb_store(s_qpark.hb + 9, rim_bits(n));
            }
            int st = 0, st2 = 0;
            double val, val2;
            COOP_DIAG(const unsigned long long e0 = wall_clock64();)
            RIM_PROF_T(t_req);
            unsigned long long samples_before = 0;
            if ((a.work || P::TURBO) && lane == 0) samples_before = s_qpark.ctr.samples;     // (rounds book a request's samples too)
            P::eval2(cx, g, inner, &s_qpark, n, lb, n2, lb2, k2 >= 0, val, st, val2, st2);
            // Work counters count what went INTO the stored value: a request evaluated for the board is booked by
            // the owner when it reads the result, so a batch the owner gives up on and evaluates again is counted once.
            unsigned long long samples_taken = 0;
            if ((a.work || P::TURBO) && lane == 0) {
                samples_taken = s_qpark.ctr.samples - samples_before;
                if (a.work && !shared) atomicAdd(a.work + own_i * 8 + (size_t) own_slot, samples_taken);
            }
            RIM_PROF_ADD(9, t_req);
            COOP_DIAG(eval_ticks += wall_clock64() - e0;)
            if (shared) {
                if (lane == 0) {
                    bput(&src->res[k], rim_bits(val));
                    bput(&src->res_status[k], st);
                    if (a.work || P::TURBO) bput(&src->res_samples[k], (unsigned) samples_taken);
                    drain_vmem();
                    __hip_atomic_fetch_add(&src->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                if (lane == k) gval = val;
                if (lane == k2) gval = val2;
                batch_status |= st | st2;
            }
        }
        if (helper) break;

        // ---------- owner: collect a shared batch ----------
        if (shared) {
            const unsigned want = (unsigned) (__builtin_popcountll(mask) * round_n);
            const int rank = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
            bool complete = false;
            const unsigned long long t0 = wall_clock64();
            for (;;) {
                unsigned dn = 0;
                if (lane == 0) dn = __hip_atomic_load(&my->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                dn = (unsigned) __builtin_amdgcn_readfirstlane((int) dn);
                if (dn >= want) {
                    complete = true;
                    COOP_DIAG(const unsigned long long w = wall_clock64() - t0; wait_ticks += w; if (w > max_wait) max_wait = w;)
                    break;
                }
                if (wall_clock64() - t0 > a.owner_ticks) break;
                __builtin_amdgcn_s_sleep(32);
            }
            if (lane == 0)
                __hip_atomic_store(&my->claim, (unsigned long long) seq << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (complete) {
                int stl = 0;
                if ((mask >> lane) & 1ull) {
                    gval = rim_frombits(bget(&my->res[rank]));
                    stl = bget(&my->res_status[rank]);
                    if (a.work) atomicAdd(a.work + own_i * 8 + (size_t) own_slot, (unsigned long long) bget(&my->res_samples[rank]));
                }
                if (wv_ballot((stl & ST_INNER_FAIL) != 0)) batch_status |= ST_INNER_FAIL;
                if (wv_ballot((stl & ST_STORE_FULL) != 0)) batch_status |= ST_STORE_FULL;
            } else {
                // A claimed request has not come back within the bound (a helper wave that is not running: the GPU is
                // shared, or part of the grid is not resident).  The value of a request does not depend on who
                // evaluates it, so the owner closes the batch and evaluates ALL of it itself -- same bits, only later --
                // and never publishes again: whatever a late helper still writes to this slot is never read.
                board_dead = true;
                shared = false;
                if (P::TURBO && round_n > 1) {
                    __syncthreads();
                    if (lane == 0) P::round_drop(s_stash);
                    __syncthreads();
                    round_n = 1;
                }
                local_mask = mask;
                batch_status = 0;
                gval = 0.;
                redo = true;
            }
        }
        } while (redo);
        if (helper) {
            if (got == 0) {
                // every request of that batch was already taken: back off before looking again
                // (last_hint is not set here: the claim word is re-read on the next poll, and that
                // poll files the hint away once the batch shows no open request)
                COOP_DIAG(n_empty_claims += 1;)
                for (int w = 0; w < backoff; w++) __builtin_amdgcn_s_sleep(127);
                if (backoff < 16) backoff *= 2;
            } else {
                if (lane == 0) __hip_atomic_fetch_add(flag_idle, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                counted_idle = true;
            }
            continue;
        }
        __syncthreads();
        {
            typename P::Task T = s_park;
            P::uniformize(T);
            unsigned long long stash_samples = 0, dropped_samples = 0;
            P::consume(cx, g, outer, T, B, gval, uni(batch_status), P::TURBO ? &s_stash : nullptr, &stash_samples, &dropped_samples, my,
                       __builtin_popcountll(mask & ((1ull << lane) - 1ull)), __builtin_popcountll(mask));
            if (P::TURBO) {
                // (work counters count what went INTO the stored value: a bisection booked from the stash brings its samples)
                if (a.work && lane == 0 && stash_samples) atomicAdd(a.work + own_i * 8 + (size_t) own_slot, stash_samples);
                // the launch's sample count is the reference's: what was evaluated ahead and never asked for comes off it
                // (counted by whichever wave evaluated it; the counters are summed modulo 2^64 at the end of the launch)
                if (dropped_samples && lane == 0) s_qpark.ctr.samples -= dropped_samples;
            }
            __syncthreads();
            if (lane == 0) s_park = T;
            __syncthreads();
        }
    }

    RIM_PROF_ADD(0, t_kernel);
#if defined(RIM_TAIL_DIAG)
    if (g.lane == 0) atomicMax(a.queue + (P::QUEUE ? 11 : 13), wall_clock64());
#endif
    __syncthreads();
#if defined(RIM_PROF) && defined(__HIP_DEVICE_COMPILE__)
    if (threadIdx.x < 32) g_rim_prof[(size_t) blockIdx.x * 32 + threadIdx.x] += rim_prof_lds[threadIdx.x];
#endif
    if (g.lane == 0) {
        atomicAdd(queue + 1, s_qpark.ctr.samples);
        atomicAdd(queue + 2, s_qpark.ctr.steps);
        atomicAdd(queue + 3, s_qpark.ctr.inner_qags);
#if defined(RIM_COOP_DIAG)
        atomicAdd(a.queue + 8, n_shared_batches);
        atomicAdd(a.queue + 9, n_helper_reqs);
        atomicAdd(a.queue + 10, n_owner_shared_reqs);
        atomicAdd(a.queue + 11, wait_ticks);
        atomicAdd(a.queue + 12, n_polls_total);
        atomicAdd(a.queue + 13, n_empty_claims);
        atomicAdd(a.queue + 14, eval_ticks);
        (void) max_wait;          // [15] is the heaviest task: (batches << 40) | point index
#endif
    }
}

template <int KIND>
__global__ __launch_bounds__(64) void gamma_integral_kernel(PointArgs pa, const double *norm_ptr, size_t count,
                                                            const double *nvals, double *out, double *spill_base)
{
    __shared__ double s_tab[96];
    __shared__ double s_inner[RIM_ISTORE_DOUBLES(CAP_INNER)];
    const GKLane g = gk_lane_init(s_tab);
    const IStore inner = istore_carve(s_inner, CAP_INNER, spill_base + (size_t) blockIdx.x * SPILL_DOUBLES_PER_WAVE, SPILL_INNER);
    __shared__ QagPark s_qpark;
    if (threadIdx.x == 0) { s_qpark.ctr = WaveCounters{0, 0, 0}; s_qpark.hb = nullptr; }
    const SymPoint pt = sym_point_of(pa);
    const DistParams d = dist_of<KIND>(pa, norm_ptr[0]);
    for (size_t i = blockIdx.x; i < count; i += gridDim.x) {
        const double n = nvals[i];
        LeungOrder ord_tmp[2];
        SymOrder so = sym_order(n, ord_tmp);
        __syncthreads();
        if (g.lane == 0) { s_qpark.ord[0] = ord_tmp[0]; s_qpark.ord[1] = ord_tmp[1]; }
        __syncthreads();
        so.o = s_qpark.ord;
        const GammaLimits L = gamma_limits(pt, n, pa.negative_lobe);
        auto f = [&](double x, bool active) -> double { return active ? gamma_integrand<KIND>(pt, d, so, x) : 0.; };
        QagState q;
        wave_qag(f, g, inner, L.g0, L.g1, 0., 1e-3, 5000, q, &s_qpark);
        if (g.lane == 0) out[i] = (q.status == QAG_SUCCESS) ? q.result : RIM_NAN;
    }
}

template <int KIND>
__global__ void integrand_kernel_n(PointArgs pa, const double *norm_ptr, size_t count, const double *n,
                                   const double *gamma, double *out)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const SymPoint pt = sym_point_of(pa);
    const DistParams d = dist_of<KIND>(pa, norm_ptr[0]);
    LeungOrder ord[2];
    const SymOrder so = sym_order(n[i], ord);
    out[i] = gamma_integrand<KIND>(pt, d, so, gamma[i]);
}

#endif
