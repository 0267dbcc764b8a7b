// rimphony_internal.h -- what the translation units of librimphony_hip.so share (not installed).
//
// The diagnostic kernels live in their own translation unit (rimphony_diag.hip): with them in the same unit as
// coop_kernel, hipcc's code generation for coop_kernel changes (87 -> 113 spilled VGPRs, +1.4 % run time,
// measured), although they share no non-inlined code.
#ifndef RIMPHONY_INTERNAL_H
#define RIMPHONY_INTERNAL_H

#include <hip/hip_runtime.h>
#include <optional>
#include <type_traits>
#include "../../include/rimphony_hip.h"
#include "symphony_wave.h"

// LDS subinterval-store capacities.  Largest counts seen on the reference's golden file and
// on the bench tables: 31 (gamma integrals), 41 (n chunks), 48 (normalisation).
#ifndef CAP_INNER
#define CAP_INNER 64
#endif
#ifndef CAP_OUTER
#define CAP_OUTER 64
#endif
#define CAP_NORM 256
// per-wave global spill behind the LDS stores: the GSL limits of the path (5000 inner for
// Symphony, 4096 for Heyvaerts, 1000 / 4096 outer)
#define SPILL_INNER 5000
#define SPILL_OUTER 4096
#define SPILL_DOUBLES_PER_WAVE (RIM_ISTORE_DOUBLES(SPILL_INNER) + RIM_ISTORE_DOUBLES(SPILL_OUTER))
// minimum waves per SIMD the register allocator must leave room for (symphony kernel)
// (measured on MI355X, 65536-point launches: 4 -> 25.8k, 5 -> 27.0k, 6 -> 27.8k points/s; at 6 the
// allocator spills 47 VGPRs to scratch and still wins)
#ifndef RIM_SYM_WAVES
#define RIM_SYM_WAVES 6
#define RIM_HEY_WAVES 5          // heyvaerts: 96 VGPRs (2..6 measured: 869, 708, 653, 626, 646 ms on the 8192-point power-law batch;
                                 // final build, 4 / 5 / 6: 782 / 741 / 718 ms on 16384 power-law points but 993 / 967 / 996 ms on 4096
                                 // pitchy-kappa points, whose tail is sequential -- 5 kept)
#endif

// waves of the Faraday kernel's grid that serve the launch's longest outer quadrature from the start (coop_common.h,
// SymArgs::early_squad), for the kinds that have such chains (HeyvaertsProblem::EARLY_SQUAD); RIMPHONY_EARLY_SQUAD
// overrides for every kind, 0 = off
#ifndef RIM_EARLY_SQUAD_DEFAULT
#define RIM_EARLY_SQUAD_DEFAULT 64
#endif

#if defined(RIM_PROF)
#define RIM_DYN_LDS 256             // the region timers accumulate in dynamic LDS
#else
#define RIM_DYN_LDS 0
#endif
// A failed HIP call: remember what failed where rimphony_last_error() can find it (thread-local; a library does
// not print) and return RIMPHONY_EHIP.
void rim_set_last_error(const char *what, const char *detail);
#define HIP_TRY(expr)                                                            \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            rim_set_last_error(#expr, hipGetErrorString(e_));                    \
            return RIMPHONY_EHIP;                                                \
        }                                                                        \
    } while (0)


struct PointArgs {
    double par[5];
    double s, theta;
    int coeff, stokes, negative_lobe;
};
// what the seam kernels make of it: the point, and the distribution with the normalisation the host left in norm[0]
__device__ __forceinline__ rim::SymPoint sym_point_of(const PointArgs &pa)
{
    rim::SymPoint pt;
    pt.s = pa.s;
    rim_sincos(pa.theta, &pt.sin_th, &pt.cos_th);
    pt.coeff = pa.coeff;
    pt.stokes = pa.stokes;
    return pt;
}
template <int KIND>
__device__ __forceinline__ rim::DistParams dist_of(const PointArgs &pa, double norm)
{
    rim::DistParams d;
    for (int k = 0; k < 5; k++) d.par[k] = pa.par[k];
    rim::dist_prepare<KIND>(d, norm);
    return d;
}

// Every entry point that touches the context's workspace (norms, spill regions, staging buffers, queue words) runs
// inside one of these: the context's (recursive) host lock for the whole call -- staging, launches, synchronisation and
// copy-out included --, the device selected, `st` ordered behind the previous call's work on the workspace, and that
// call's own last kernel recorded for the next one when the scope ends.  enter() also forgets the thread's previous
// error text, so that rimphony_last_error() never describes an older call.
void rim_ctx_lock(rimphony_ctx *c);
void rim_ctx_unlock(rimphony_ctx *c);
int rim_ctx_enter(rimphony_ctx *c, hipStream_t st);
void rim_ctx_leave(rimphony_ctx *c, hipStream_t st);
void rim_clear_last_error();
struct RimCtxScope {
    rimphony_ctx *c;
    hipStream_t st;
    bool entered;
    RimCtxScope(rimphony_ctx *ctx, hipStream_t stream) : c(ctx), st(stream), entered(false) { rim_ctx_lock(c); }
    int enter() { const int rc = rim_ctx_enter(c, st); entered = (rc == 0); return rc; }
    ~RimCtxScope() { if (entered) rim_ctx_leave(c, st); rim_ctx_unlock(c); }
    RimCtxScope(const RimCtxScope &) = delete;
    RimCtxScope &operator=(const RimCtxScope &) = delete;
};

// The one way into the eight per-point seams (one host-described parameter point, arrays of abscissae).  begin(), in this
// order: the point validated on the host (kind, params, coeff and stokes ranges, a table set for the tabulated kind) before
// any lock or HIP call; count == 0 is RIMPHONY_OK with nothing enqueued; then the scope (lock, device, ordering), the
// point's normalisation into norm[0], and the grid: waves_per_cu == 0 is one thread per item in blocks of 64, anything else a
// persistent grid of single-wave workgroups with its region of `spill`.  `kind` is the instantiation that serves the
// point: the form of the installed table set as rim_tab_seam_kind reads it for RIMPHONY_TABULATED, the kind itself
// otherwise.  The entry then launches on `st` and asks hipGetLastError(); the scope ends with the object.
struct RimPointSeam {
    std::optional<RimCtxScope> scope;
    PointArgs pa;
    hipStream_t st;
    unsigned grid;
    const double *norm;
    double *spill;
    int kind;
    int begin(rimphony_ctx *c, int kind, const double *params, int coeff, int stokes, int negative_lobe, double s, double theta,
              size_t count, int waves_per_cu, void *stream);
};

// The one place where a run-time distribution kind picks a template instantiation: f(std::integral_constant<int, K>{}).
// Every entry has validated `kind` before, so anything else is kind 3 (the tabulated distribution never gets here:
// rim_with_tab_kind below).
template <class F>
auto rim_with_kind(int kind, F &&f)
{
    switch (kind) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
    }
}

// The same for the tabulated distribution, whose instantiations go by the form of the installed table set: the set's
// DIST_TABULATED* value (dev_symphony.h), which is what a context remembers, the cell of its occupancy caches and the
// argument of tab_launch.h.  Anything but the fifteen named forms is DIST_TABULATED, a set with pitch rows.
template <class F>
auto rim_with_tab_kind(int tab_kind, F &&f)
{
    using namespace rim;
    switch (tab_kind) {
    case DIST_TABULATED_ISO: return f(std::integral_constant<int, DIST_TABULATED_ISO>{});
    case DIST_TABULATED_2D: return f(std::integral_constant<int, DIST_TABULATED_2D>{});
    case DIST_TABULATED_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_PITCHY>{});
    case DIST_TABULATED_GRID: return f(std::integral_constant<int, DIST_TABULATED_GRID>{});
    case DIST_TABULATED_2D_GRID: return f(std::integral_constant<int, DIST_TABULATED_2D_GRID>{});
    case DIST_TABULATED_2D_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_PITCHY>{});
    case DIST_TABULATED_2D_GRID_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_GRID_PITCHY>{});
    case DIST_TABULATED_2D_NODES: return f(std::integral_constant<int, DIST_TABULATED_2D_NODES>{});
    case DIST_TABULATED_2D_NODES_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_NODES_PITCHY>{});
    case DIST_TABULATED_FAMILY: return f(std::integral_constant<int, DIST_TABULATED_FAMILY>{});
    case DIST_TABULATED_FAMILY_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_FAMILY_PITCHY>{});
    case DIST_TABULATED_2D_FAMILY: return f(std::integral_constant<int, DIST_TABULATED_2D_FAMILY>{});
    case DIST_TABULATED_2D_FAMILY_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_FAMILY_PITCHY>{});
    case DIST_TABULATED_2D_FAMILY_CUBIC: return f(std::integral_constant<int, DIST_TABULATED_2D_FAMILY_CUBIC>{});
    case DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>{});
    default: return f(std::integral_constant<int, DIST_TABULATED>{});
    }
}

// Only coop_kernel and group_kernel have an instantiation for DIST_TABULATED_ISO (the persistent kernels keep the code
// isotropic tables always ran); every other kernel reads a set without pitch rows with its DIST_TABULATED instantiation,
// same bits.  This is the one place that says so.
constexpr int rim_tab_seam_kind(int tab_kind) { return tab_kind == rim::DIST_TABULATED_ISO ? (int) rim::DIST_TABULATED : tab_kind; }

// rim_with_kind for the translation units whose kernels serve all kinds (RimPointSeam::kind supplies `kind`).
// rimphony_group.hip keeps the four-way form: its kernels exist for the four analytic kinds only; the tabulated kind's
// group kernels are reached through tab_launch.h (rim_tab_group_kernel).
template <class F>
auto rim_with_kind5(int kind, F &&f)
{
    if (!rim::dist_is_tab(kind)) return rim_with_kind(kind, f);
    return rim_with_tab_kind(kind, [&](auto K) { return f(std::integral_constant<int, rim_tab_seam_kind(decltype(K)::value)>{}); });
}

// Leaves the calling thread on the device it came with, whichever way the scope ends.
struct RimDeviceScope {
    int device;
    RimDeviceScope() : device(-1) { if (hipGetDevice(&device) != hipSuccess) device = -1; }
    ~RimDeviceScope() { if (device >= 0) (void) hipSetDevice(device); }
    RimDeviceScope(const RimDeviceScope &) = delete;
    RimDeviceScope &operator=(const RimDeviceScope &) = delete;
};

#endif
