// rimphony_group.hip -- group_kernel<P> (group_kernel.h) for the four analytic distributions: the Symphony coefficients of a
// parameter point in lock-step, and the Faraday pair's problem (gfx950 only).
//
// A translation unit of its own: hipcc's code generation for a kernel of this size depends on what else is in the
// unit (rimphony_internal.h).  The tabulated distribution's instantiations live in rimphony_tab_group.hip for the same
// reason; this unit keeps the four-way dispatch.
#include "group_kernel.h"

// ---- the Faraday pair in lock-step (heyvaerts_group.h); the Symphony groups' problem is in group_kernel.h ---------
template <int KIND>
struct HeyGroupProblem {
    typedef HeyTask Task;
    typedef GroupParkBase Park;
    struct Ctx { HeyPoint pt; DistParams d; HeyConsts hc; };
    enum : int { QUEUE = 4, TAIL_WORD = 15, STATS_WORD = 10, WAVES = RIM_HEY_GROUP_WAVES, EXTRA_LDS_DOUBLES = 1,
                 GSPILL_OUTER = SPILL_HEYGOUTER, SPILL_PER_WAVE = SPILL_HEYGROUP_DOUBLES_PER_WAVE };
    static __device__ __forceinline__ void init(const SymArgs &a, Ctx &c, double *extra_lds)
    {
        c.hc = hey_consts();
        c.pt.s = 0.; c.pt.cos_th = 0.; c.pt.sin_th = 0.; c.pt.sigma0 = 0.; c.pt.sigma0_sq = 0.; c.pt.dinv = 0.; c.pt.endless_gamma = RIM_INF; c.pt.stokes = STOKES_Q;
    }
    static __device__ __forceinline__ void load(const SymArgs &a, size_t i, unsigned, Ctx &c, double &norm)
    {
        HeyPoint &pt = c.pt;
        pt.s = uni(a.s[i]);
        rim_sincos(a.theta[i], &pt.sin_th, &pt.cos_th);
        pt.sin_th = uni(pt.sin_th);
        pt.cos_th = uni(pt.cos_th);
        hey_point_derive(pt);
        pt.sigma0 = uni(pt.sigma0); pt.sigma0_sq = uni(pt.sigma0_sq); pt.dinv = uni(pt.dinv);
        pt.stokes = STOKES_Q;
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
    static __device__ __forceinline__ HeyPoint member_point(const Ctx &c, int slot)
    { HeyPoint pt = c.pt; pt.stokes = hey_slot_stokes(slot); return pt; }
    static __device__ __forceinline__ void begin(const Ctx &c, int slot, Task &T) { hey_begin(member_point(c, slot), T); }
    static __device__ __forceinline__ void uniformize(Task &T) { hey_uniformize(T); }
    static __device__ __forceinline__ bool done(const Task &T) { return T.stage == HS_DONE; }
    static __device__ __forceinline__ int batches(const Task &T) { return T.batches; }
    static __device__ __forceinline__ bool post(const Ctx &c, int slot, const GKLane &g, const IStore &outer, Task &T, SymBatch &B)
    { return hey_post(member_point(c, slot), g, outer, T, B); }
    static __device__ __forceinline__ void consume(const Ctx &c, int slot, const GKLane &g, const IStore &outer, Task &T,
                                                   const SymBatch &B, double gval, int bst)
    { hey_consume(member_point(c, slot), g, outer, T, B, gval, bst); }
    static __device__ __forceinline__ double result(const Ctx &, int, const Task &T, int &st) { return hey_result(T, st); }
    static __device__ __forceinline__ unsigned turn(const Task *park, unsigned alive) { return hey_group_turn(park, alive); }
    static __device__ __forceinline__ void eval(const Ctx &c, unsigned slots, const GKLane &g, double *lds, double *spill, Park *gp,
                                                double x0, int t0, unsigned m0, double x1, int t1, unsigned m1)
    { hey_eval_group<KIND>(c.pt, c.d, c.hc, slots, g, lds, spill, gp, x0, t0, m0, x1, t1, m1); }
};

// ---- launch interface (group_launch.h) -----------------------------------------------------------------------
const void *rim_group_kernel(int kind, int faraday)
{
    return rim_with_kind(kind, [&](auto K) -> const void * {
        constexpr int KIND = decltype(K)::value;
        return faraday ? reinterpret_cast<const void *>(group_kernel<HeyGroupProblem<KIND>>)
                       : reinterpret_cast<const void *>(group_kernel<SymGroupProblem<KIND>>);
    });
}

int rim_group_waves(int faraday) { return faraday ? RIM_HEY_GROUP_WAVES : RIM_GROUP_WAVES; }
