// rimphony_hip.hip -- kernels and C ABI of librimphony_hip.so (gfx950 only).
//
// Kernels (one 64-lane wavefront per workgroup; each wave owns its LDS):
//   norm_kernel<KIND>      full_calculation(): per-point normalisation integral
//   coop_kernel<P>         (point, coefficient) tasks pulled from an atomic queue, with a cooperative tail;
//                          P = SymphonyProblem<KIND> (j, alpha) or HeyvaertsProblem<KIND> (rho_Q, rho_V)
//                          (both templates: coop_kernel.h; this unit instantiates them for the four analytic distributions,
//                          rimphony_tab.hip for the tabulated one)
//   highfreq_kernel        closed-form high-frequency rho_Q, rho_V
//   bessel_kernel, integrand_kernel, gamma_integral_kernel, qag_selftest_kernel
//                          unit seams used by the parity tests
//
// Launch geometry: a persistent grid of RIM_WAVES_PER_CU x 256 single-wave
// workgroups; per-task cost spans orders of magnitude, so
// tasks are handed out dynamically, one atomicAdd per task.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include <mutex>
#include <thread>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>
#include "../../include/rimphony_hip.h"
#include "symphony_wave.h"
#include "heyvaerts_wave.h"
#include "highfreq.h"

using namespace rim;

#include "rimphony_internal.h"
#include "coop_common.h"
#include "group_launch.h"
#include "launch_plan.h"

#include "coop_kernel.h"
#include "tab_launch.h"
#include "tab_spline.h"

__global__ void board_init_kernel(unsigned *flags, unsigned active)
{
    const unsigned i = threadIdx.x;
    if (blockIdx.x == 0)
        for (unsigned k = i; k < BOARD_FLAG_WORDS; k += blockDim.x) flags[k] = (k == BOARD_FLAG_ACTIVE) ? active : 0u;
}

// ------------------------------------------------------------------------------
// heyvaerts (Faraday rho_Q = slot 6, rho_V = slot 7)
// ------------------------------------------------------------------------------

// ------------------------------------------------------------------------------
// expensive-first task order.  The cost of a point grows with s (about 3x from s < 10 to
// s > 100 on the bench tables), so points are bucketed by the binary exponent of s and the
// persistent grid starts with the large-s buckets: the cheap points then fill the tail of the
// launch.  Only the order of evaluation changes, never a result.
// ------------------------------------------------------------------------------
#define ORDER_BUCKETS 32

// The Faraday kernel's tasks have their own cost profile (per-coefficient batch counts of a -DRIM_TAIL_DIAG build, round 4,
// all four tables): the fewer harmonics -- the smaller sigma0 = s sin(theta) -- the MORE batches (mean 37 at the top decile
// of s, 67 at the bottom one; 200+ at sigma0 ~ 0.005), and the outer quadratures that run to GSL's limit of 4096
// bisections (heyvaerts.rs:82-83; one task in ~1e5, thousands of sequential batches) all sat at sigma0 in [1.15, 2.4]
// (power law: 2.15, 2.40; pitchy kappa: 1.15, 1.20, 1.41).  With the Symphony order (large s first) exactly these tasks
// started last.  Here: the window 0.9 <= sigma0 <= 3 first (10 % of the rows; a chain that starts with the launch has
// the whole launch to overlap with -- coop_common.h, early help), then ascending sigma0.
__device__ __forceinline__ int faraday_order_bucket(double s, double theta)
{
    double sn, cs;
    rim_sincos(theta, &sn, &cs);
    const double sigma0 = s * rim_fabs(sn);
    if (sigma0 >= 0.9 && sigma0 <= 3.) return 0;
    if (!(sigma0 > 0.)) return ORDER_BUCKETS - 1;
    const int e = (int) ((rim_bits(sigma0) >> 52) & 0x7ff) - 1023;     // floor(log2 sigma0) for normal sigma0
    const int b = e + 11;                                                // sigma0 < 2^-10 -> 1, ..., sigma0 >= 2^19 -> 31
    return b < 1 ? 1 : (b > ORDER_BUCKETS - 1 ? ORDER_BUCKETS - 1 : b);
}

__device__ __forceinline__ int order_bucket(double s, double theta, const double *gmin, const double *temp, size_t i, int faraday)
{
    if (faraday) return faraday_order_bucket(s, theta);
    // Thermal distribution: the long tasks are the COLD, LOW-FREQUENCY, SMALL-ANGLE points, not the large-s ones -- there
    // j_V / alpha_V march through ~300 batches of the tail integral before GSL's round-off detector ends them (NaN, as in
    // the reference), ten times the table's median.  Measured on 65536 rows of configs[2]'s table with the per-coefficient
    // batch counts of a -DRIM_TAIL_DIAG build (round 4): s sin(theta) T^2 < 1 holds for 18 % of the rows and 95 % of the
    // coefficients of 200 batches and more (< 0.01: 3 % of the rows, 43 % of them, 92 % pure).  They go first; with the
    // large-s-first order they started last and were 12 % of a 65536-row launch of the Symphony groups.
    if (temp) {
        double sn, cs;
        rim_sincos(theta, &sn, &cs);
        const double t = temp[i];
        const double key = s * rim_fabs(sn) * (t * t);
        if (key < 0.01) return 0;
        if (key < 0.1) return 1;
        if (key < 1.) return 2;
        const int e = (int) ((rim_bits(s) >> 52) & 0x7ff) - 1023;
        const int b = 17 - e;
        return b < 3 ? 3 : (b > ORDER_BUCKETS - 1 ? ORDER_BUCKETS - 1 : b);
    }
    // Points whose 30 discrete harmonics all lie below gamma_min (power-law families) start the n
    // integration from zero and must resolve the onset at gamma_min inside one wide chunk: they are
    // 100-1000x the mean cost (and usually end in a GSL round-off failure, as in the reference).
    // They go first.
    if (gmin) {
        double sn, cs;
        rim_sincos(theta, &sn, &cs);
        const double n = rim_floor(s * rim_fabs(sn) + 30.);
        const double nos = n / s;
        const double gp = (nos + rim_fabs(cs) * rim_sqrt(nos * nos - sn * sn)) / (sn * sn);
        if (gp < gmin[i]) return 0;
    }
    const int e = (int) ((rim_bits(s) >> 52) & 0x7ff) - 1023;     // floor(log2 s) for normal s
    int b = 17 - e;                                                 // large s -> small bucket index
    return b < 1 ? 1 : (b > ORDER_BUCKETS - 1 ? ORDER_BUCKETS - 1 : b);
}

__global__ void order_hist_kernel(const double *s, const double *theta, const double *gmin, const double *temp, size_t n, unsigned *hist,
                                  int faraday)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&hist[order_bucket(s[i], theta[i], gmin, temp, i, faraday)], 1u);
}

__global__ void order_scan_kernel(unsigned *hist)   // exclusive scan in place, one thread
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        unsigned acc = 0;
        for (int b = 0; b < ORDER_BUCKETS; b++) { const unsigned c = hist[b]; hist[b] = acc; acc += c; }
    }
}

__global__ void order_scatter_kernel(const double *s, const double *theta, const double *gmin, const double *temp, size_t n,
                                     unsigned *offsets, unsigned *perm, int faraday)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[atomicAdd(&offsets[order_bucket(s[i], theta[i], gmin, temp, i, faraday)], 1u)] = (unsigned) i;
}

// fills the slots that were not selected (or not yet available) with NaN
__global__ void fill_unselected_kernel(double *out, int32_t *status, size_t n, uint32_t computed_mask)
{
    const size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * 8) return;
    const int slot = (int) (idx & 7);
    if (!(computed_mask & (1u << slot))) {
        out[idx] = RIM_NAN;
        if (status) status[idx] = ST_NONFINITE | RIMPHONY_ST_NOT_COMPUTED;
    }
}

// ------------------------------------------------------------------------------
// unit seams
// ------------------------------------------------------------------------------

__global__ void bessel_kernel(size_t count, const double *n, const double *x, double *j, double *dj)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    if (j) j[i] = bessel_j(n[i], x[i]);
    if (dj) dj[i] = bessel_dj(n[i], x[i]);
}


__device__ inline double selftest_integrand(int family, double p0, double p1, double x)
{
    switch (family) {
    case 0: { const double u = (x - p0) * p1; return 1. / (1. + u * u); }
    case 1: return rim_sqrt(rim_fabs(x - p0)) * p1;
    case 2: return x * x * (p0 + x * p1);
    case 3: return 1. / rim_sqrt(rim_fabs(x - p0) + p1);
    default: { const double u = x * p0; return p1 * rim_fabs((u - rim_floor(u)) - 0.5); }   // triangle wave: long lists
    }
}

__global__ __launch_bounds__(64) void qag_selftest_kernel(size_t count, const int32_t *family, const double *p0,
                                                          const double *p1, const double *a, const double *b,
                                                          double epsabs, double epsrel, int limit,
                                                          double *result, double *abserr, int32_t *qstatus, int32_t *size,
                                                          double *spill_base)
{
    __shared__ double s_tab[96];
    __shared__ double s_store[RIM_ISTORE_DOUBLES(CAP_NORM)];
    const GKLane g = gk_lane_init(s_tab);
    const IStore st = istore_carve(s_store, CAP_NORM, spill_base + (size_t) blockIdx.x * SPILL_DOUBLES_PER_WAVE, SPILL_INNER);
    __shared__ QagPark s_qpark;
    if (threadIdx.x == 0) { s_qpark.ctr = WaveCounters{0, 0, 0}; s_qpark.hb = nullptr; }
    // problems 2j and 2j + 1 run as a pair (wave_qag_pair: shared first rule application), as the
    // product kernels run their gamma-integrals; an odd last problem runs alone
    for (size_t i = 2 * (size_t) blockIdx.x; i < count; i += 2 * (size_t) gridDim.x) {
        const bool have1 = i + 1 < count;
        const size_t i1 = have1 ? i + 1 : i;
        const int fam0 = family[i], fam1 = family[i1];
        const double q00 = p0[i], q01 = p1[i], q10 = p0[i1], q11 = p1[i1];
        auto f = [&](double x, bool active, bool second) -> double {
            return active ? selftest_integrand(second ? fam1 : fam0, second ? q10 : q00, second ? q11 : q01, x) : 0.;
        };
        double r0, r1, ae[2];
        int s0, s1, sz[2];
        wave_qag_pair(f, g, st, a[i], b[i], a[i1], b[i1], have1, false, epsabs, epsrel, limit, &s_qpark, r0, s0, r1, s1, ae, sz);
        if (g.lane == 0) {
            result[i] = r0; abserr[i] = ae[0]; qstatus[i] = s0; size[i] = sz[0];
            if (have1) { result[i1] = r1; abserr[i1] = ae[1]; qstatus[i1] = s1; size[i1] = sz[1]; }
        }
    }
}

// ------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------

// A device buffer of the context's workspace.  It only ever grows; `cap` counts what its user counts (points, waves,
// board slots).  A failed growth leaves it empty, so that a smaller call can still be served.
template <class T>
struct RimDevBuf {
    T *p;
    size_t cap;
    void release()
    {
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // room for n elements in `bytes` bytes; `what` names the buffer in the error text
    int grow(size_t n, size_t bytes, const char *what)
    {
        if (cap >= n) return RIMPHONY_OK;
        release();
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void) hipGetLastError();       // reported here: it must not stick to the next HIP call
            p = nullptr;
            char msg[200];
            snprintf(msg, sizeof msg, "%zu MB for %s", bytes >> 20, what);
            rim_set_last_error("hipMalloc", msg);
            return RIMPHONY_ENOMEM;
        }
        cap = n;
        return RIMPHONY_OK;
    }
};

// ---- the knobs: environment variables read once, when a context is created (DESIGN.md "Environment variables") ----
struct RimKnobs {
    long long no_assist, sym_solo, faraday_symphony_order, rounds, early_squad, early_min, f32_variant, faraday_group, owner_wait_us,
              tab_group;
};
enum RimKnobKind {
    KNOB_ON_1,          // on when the value starts with '1'
    KNOB_OFF_0,         // on unless the value starts with '0'
    KNOB_LETTER,        // on when the value starts with the letter in `lo`
    KNOB_INT,           // atoi of the value (also of an empty one), clamped to [lo, hi]
    KNOB_U64            // strtoull of a non-empty value
};
struct RimKnobDef {
    const char *name;
    RimKnobKind kind;
    long long RimKnobs::*field;
    long long dflt, lo, hi;
    const char *text;
};
static const RimKnobDef RIM_KNOBS[] = {
    { "RIMPHONY_NO_ASSIST", KNOB_ON_1, &RimKnobs::no_assist, 0, 0, 0,
      "=1: one wave per task to the end, no cooperative tail (A/B measurements)" },
    { "RIMPHONY_SYM_SOLO", KNOB_ON_1, &RimKnobs::sym_solo, 0, 0, 0,
      "=1: one wave per (point, coefficient) for the Symphony slots, the round-2 kernel (A/B measurements)" },
    { "RIMPHONY_FARADAY_ORDER", KNOB_LETTER, &RimKnobs::faraday_symphony_order, 0, 's', 0,
      "=symphony: the Faraday launch visits the points in the Symphony order (A/B measurements)" },
    { "RIMPHONY_ROUNDS", KNOB_OFF_0, &RimKnobs::rounds, 1, 0, 0,
      "=0: a long outer quadrature evaluates one interval per batch, as until round 4 (A/B measurements)" },
    { "RIMPHONY_EARLY_SQUAD", KNOB_INT, &RimKnobs::early_squad, -1, INT_MIN, 1024,
      "waves of the Faraday grid that serve the longest chain from the start (0: off; unset or negative: the kind's default)" },
    { "RIMPHONY_EARLY_MIN", KNOB_INT, &RimKnobs::early_min, 16, 1, INT_MAX,
      "batches after which a task competes for that help" },
    { "RIMPHONY_F32_VARIANT", KNOB_ON_1, &RimKnobs::f32_variant, 0, 0, 0,
      "=1: accept RIMPHONY_PRECISION_F32_INTEGRAND (measurement hook)" },
    { "RIMPHONY_FARADAY_GROUP", KNOB_ON_1, &RimKnobs::faraday_group, 0, 0, 0,
      "=1: rho_Q and rho_V of a point in lock-step (measured slower: DESIGN.md section 5)" },
    { "RIMPHONY_OWNER_WAIT_US", KNOB_U64, &RimKnobs::owner_wait_us, 120000000, 0, 0,
      "microseconds an owner waits for its helpers before it recomputes a batch itself (test hook; 0 is accepted)" },
    { "RIMPHONY_TAB_GROUP", KNOB_INT, &RimKnobs::tab_group, -1, INT_MIN, 1,
      "Symphony slots of the tabulated kind: 1 = in lock-step on the group kernel, 0 = one wave per coefficient, for every form (unset or negative: the form's default)" },
};

static RimKnobs rim_read_knobs()
{
    RimKnobs k;
    for (const RimKnobDef &d : RIM_KNOBS) {
        const char *e = getenv(d.name);
        long long v = d.dflt;
        switch (d.kind) {
        case KNOB_ON_1: v = (e && e[0] == '1'); break;
        case KNOB_OFF_0: v = (e && e[0] == '0') ? 0 : 1; break;
        case KNOB_LETTER: v = (e && e[0] == (char) d.lo); break;
        case KNOB_INT:
            if (e) v = atoi(e);
            if (v < d.lo) v = d.lo;
            if (v > d.hi) v = d.hi;
            break;
        case KNOB_U64: if (e && e[0]) v = (long long) strtoull(e, nullptr, 10); break;
        }
        k.*d.field = v;
    }
    return k;
}

struct rimphony_ctx {
    int device;
    int n_cu;
    RimKnobs knobs;
    int no_assist;                  // knobs.no_assist, or shared mode: one wave per task to the end
    RimDevBuf<unsigned long long> d_queue;  // 16 words
    RimDevBuf<double> d_norm;       // [cap], and with it
    RimDevBuf<unsigned> d_perm;     // [cap] task order + ORDER_BUCKETS histogram words behind it
    RimDevBuf<double> d_spill;      // [cap waves][SPILL_DOUBLES_PER_WAVE]
    RimDevBuf<char> d_board;        // [cap] AssistSlot + flag words behind
    // staging for the host-buffer entry point
    RimDevBuf<double> d_in;
    RimDevBuf<double> d_out;        // [cap][8], and with it
    RimDevBuf<int32_t> d_status;    // [cap][8] status words, then [cap][8] uint64 work counters
    // HIP events bracketing the most recent Symphony / Faraday launch
    hipEvent_t ev_start, ev_stop;   // Symphony launch
    int ev_valid;
    hipEvent_t ev_fstart, ev_fstop; // Faraday launch
    int evf_valid;
    // diagnostics: heartbeat words in host-mapped memory
    unsigned long long *hb_host;
    unsigned long long *hb_dev;
    unsigned long long hb_task;
    // what hipOccupancyMaxActiveBlocksPerMultiprocessor answered (-1: the query failed), asked once per context
    // (= per device) and instantiation: coop_kernel<P> by problem (0 Symphony, 1 Heyvaerts) and distribution kind,
    int resident[2][20];            // (kind 4 sixteen times: the cell of a table set is its DIST_TABULATED* value, tab_kind below)
    int resident_f32[4];            // ... the Symphony kernels' fp32-integrand variants,
    int resident_group[2][20];      // ... group_kernel<P> [Symphony groups / Faraday pair][kind] (kind 4: the cells of `resident`; no Faraday pair)
    // 0: this context has the GPU to itself (it holds the device's lock file); 1: another context or process had
    // the device first -- smaller persistent grids, no cooperative tail (see rimphony_ctx_create)
    int shared_mode;
    int lock_fd;
    unsigned long long ticks_per_s;  // wall_clock64 rate of the device
    unsigned long long owner_wait_ticks;   // how long an owner waits for its helpers before recomputing a batch itself
    // successive batch calls of a context share its workspace: each call's stream waits for the previous call's
    // work (ev_batch), and the calls themselves are serialised by mu
    hipEvent_t ev_batch;
    int ev_batch_valid;
    std::recursive_mutex *mu;
    // group kernel (rimphony_group.hip): per-wave spill regions and board
    RimDevBuf<double> d_gspill;     // [cap waves]
    int gspill_faraday;             // the region is sized for the Faraday pair's longer outer lists
    RimDevBuf<char> d_gboard;       // [cap] GroupSlot + flag words behind
    // the table set of the tabulated distribution (rimphony_ctx_set_tables; dev_symphony.h has the layout), or empty
    RimDevBuf<double> d_tab;
    int tab_kind = DIST_TABULATED_ISO;  // the form of that set as its DIST_TABULATED* value (tab_launch.h): which instantiation of the kind's kernels runs
    // a family with a sin^k prefactor, and a family of 2-D surfaces with one or without: one 64-byte line per row of the batch
    // in flight (dev_symphony.h: tab_family_line, tab_2d_family_line; 128 bytes where the surfaces are blended cubically:
    // tab_2d_family_cubic_line), written by the normalisation's launch and read by every later kernel of the batch
    RimDevBuf<double> d_famline;
};

// ---- last error (thread-local text; the codes are in rimphony_hip.h) ---------------------------
static thread_local char t_last_error[256] = "";
void rim_set_last_error(const char *what, const char *detail)
{
    snprintf(t_last_error, sizeof t_last_error, "%s: %s", what ? what : "?", detail ? detail : "?");
}
extern "C" const char *rimphony_last_error(void) { return t_last_error; }
void rim_clear_last_error() { t_last_error[0] = 0; }

void rim_ctx_lock(rimphony_ctx *c) { c->mu->lock(); }
void rim_ctx_unlock(rimphony_ctx *c) { c->mu->unlock(); }

extern "C" const char *rimphony_strerror(int code)
{
    switch (code) {
    case RIMPHONY_OK: return "success";
    case RIMPHONY_EINVAL: return "invalid argument";
    case RIMPHONY_EHIP: return "HIP runtime error";
    case RIMPHONY_ENOMEM: return "out of memory";
    case RIMPHONY_ENODEVICE: return "no usable HIP device (this library has no CPU fallback)";
    case RIMPHONY_EBUSY: return "the device is in use by another rimphony context (RIMPHONY_EXCLUSIVE=1)";
    case RIMPHONY_ENOTSUP: return "not supported";
    case RIMPHONY_ERCCL: return "RCCL call failed";
    default: return "unknown error";
    }
}

extern "C" const char *rimphony_version(void) { return "rimphony_hip 0.3 (gfx950)"; }

// One context per GPU is the supported configuration: the persistent grids of the two coefficient kernels fill the
// device and their idle waves help the busy ones (cooperative tail), which only works while every wave of the grid is
// resident.  Whether somebody else is on the device cannot be asked of the runtime, so contexts announce themselves:
// the first one on a device (any process) takes an exclusive flock on /dev/shm/rimphony_hip.<pci bus id>.lock and
// keeps it for its lifetime; a context that finds the lock taken runs in SHARED mode -- quarter-size grids, no
// cooperative tail, hence no wave ever waits for another -- or, with RIMPHONY_EXCLUSIVE=1, is refused (RIMPHONY_EBUSY).
static int take_device_lock(int device, int *fd_out)
{
    *fd_out = -1;
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, (int) sizeof bus, device) != hipSuccess) snprintf(bus, sizeof bus, "dev%d", device);
    for (char *q = bus; *q; q++) if (*q == ':' || *q == '/') *q = '_';
    char path[160];
    snprintf(path, sizeof path, "/dev/shm/rimphony_hip.%s.lock", bus);
    // /dev/shm is world-writable: never follow a planted symlink, only lock a regular file, and only widen the mode of
    // a file this process has just created (O_EXCL), so that another user's context can open it later.
    int fd = open(path, O_CREAT | O_EXCL | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
    if (fd >= 0) (void) fchmod(fd, 0666);
    else fd = open(path, O_RDWR | O_CLOEXEC | O_NOFOLLOW);
    if (fd < 0) return 0;                       // cannot tell: assume the device is ours
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); return 0; }
    if (flock(fd, LOCK_EX | LOCK_NB) == 0) { *fd_out = fd; return 0; }
    close(fd);
    return 1;                                   // somebody else holds it
}

static void ctx_free(rimphony_ctx *c)
{
    c->d_queue.release();
    c->d_norm.release();
    c->d_perm.release();
    c->d_spill.release();
    c->d_board.release();
    c->d_gspill.release();
    c->d_gboard.release();
    c->d_tab.release();
    c->d_famline.release();
    c->d_in.release();
    c->d_out.release();
    c->d_status.release();
    if (c->hb_host) (void) hipHostFree(c->hb_host);
    if (c->ev_start) (void) hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void) hipEventDestroy(c->ev_stop);
    if (c->ev_fstart) (void) hipEventDestroy(c->ev_fstart);
    if (c->ev_fstop) (void) hipEventDestroy(c->ev_fstop);
    if (c->ev_batch) (void) hipEventDestroy(c->ev_batch);
    if (c->lock_fd >= 0) close(c->lock_fd);     // releases the flock
    delete c->mu;
    delete c;
}

extern "C" int rimphony_ctx_create(int device, rimphony_ctx **out)
{
    if (!out) return RIMPHONY_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RIMPHONY_ENODEVICE;
    if (device < 0 || device >= ndev) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    rimphony_ctx *c = new (std::nothrow) rimphony_ctx();
    if (!c) return RIMPHONY_ENOMEM;
    memset(c, 0, sizeof *c);
    c->device = device;
    c->lock_fd = -1;
    c->mu = new (std::nothrow) std::recursive_mutex();
    if (!c->mu) { delete c; return RIMPHONY_ENOMEM; }
    c->knobs = rim_read_knobs();
    c->no_assist = c->knobs.no_assist != 0;
    c->shared_mode = take_device_lock(device, &c->lock_fd);
    if (c->shared_mode) {
        const char *e = getenv("RIMPHONY_EXCLUSIVE");
        if (e && e[0] == '1') { ctx_free(c); return RIMPHONY_EBUSY; }
        c->no_assist = 1;
    }
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {   // rate of wall_clock64() (s_memrealtime): 100 MHz on gfx950, asked rather than assumed
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
        c->ticks_per_s = (unsigned long long) khz * 1000ull;
        // 120 s; the test hook RIMPHONY_OWNER_WAIT_US shortens the bound so that the recompute path runs
        // (tests/test_gpu_boundary.py::test_owner_fallback_changes_no_bit)
        c->owner_wait_ticks = (unsigned long long) c->knobs.owner_wait_us * c->ticks_per_s / 1000000ull;
    }
    if (c->d_queue.grow(16, 16 * sizeof(unsigned long long), "the task queue words")) { ctx_free(c); return RIMPHONY_ENOMEM; }
    if (hipEventCreate(&c->ev_start) != hipSuccess || hipEventCreate(&c->ev_stop) != hipSuccess ||
        hipEventCreate(&c->ev_fstart) != hipSuccess || hipEventCreate(&c->ev_fstop) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_batch, hipEventDisableTiming) != hipSuccess) {
        ctx_free(c);
        return RIMPHONY_EHIP;
    }
    if (hipDeviceSynchronize() != hipSuccess) { ctx_free(c); return RIMPHONY_EHIP; }
    *out = c;
    return RIMPHONY_OK;
}

extern "C" void rimphony_ctx_destroy(rimphony_ctx *c)
{
    if (!c) return;
    (void) hipSetDevice(c->device);
    (void) hipDeviceSynchronize();
    ctx_free(c);
}

extern "C" int rimphony_ctx_shared_mode(const rimphony_ctx *c) { return c ? c->shared_mode : RIMPHONY_EINVAL; }
extern "C" int rimphony_ctx_device(const rimphony_ctx *c, int *device)
{
    if (!c || !device) return RIMPHONY_EINVAL;
    *device = c->device;
    return RIMPHONY_OK;
}

int rim_ctx_enter(rimphony_ctx *c, hipStream_t st)
{
    rim_clear_last_error();
    HIP_TRY(hipSetDevice(c->device));
    if (c->ev_batch_valid) HIP_TRY(hipStreamWaitEvent(st, c->ev_batch, 0));
    return RIMPHONY_OK;
}
void rim_ctx_leave(rimphony_ctx *c, hipStream_t st)
{
    // also after a failure part-way: whatever was enqueued must finish before the workspace is reused
    if (hipEventRecord(c->ev_batch, st) == hipSuccess) c->ev_batch_valid = 1;
}

static int ensure_spill(rimphony_ctx *c, size_t waves)
{
    return c->d_spill.grow(waves, waves * SPILL_DOUBLES_PER_WAVE * sizeof(double), "the subinterval spill region");
}

static int ensure_norm(rimphony_ctx *c, size_t n)
{
    if (c->d_norm.cap >= n) return RIMPHONY_OK;
    // the pair grows together
    c->d_perm.release();
    int rc = c->d_norm.grow(n, n * sizeof(double), "the normalisations");
    if (!rc) rc = c->d_perm.grow(n, (n + ORDER_BUCKETS) * sizeof(unsigned), "the visiting order");
    if (rc) c->d_norm.release();
    return rc;
}

// persistent grid: enough single-wave workgroups to fill every SIMD several times over
static unsigned persistent_grid(const rimphony_ctx *c, unsigned long long ntasks, int waves_per_cu)
{
    unsigned long long g = (unsigned long long) c->n_cu * (unsigned) waves_per_cu;
    if (g > ntasks) g = ntasks;
    if (g < 1) g = 1;
    return (unsigned) g;
}

static int launch_norm(rimphony_ctx *c, int kind, size_t n, const ParamPtrs &pp, double *d_norm, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(c->d_queue.p, 0, sizeof(unsigned long long), st));
    const unsigned grid = persistent_grid(c, n, 16);
    int rc = ensure_spill(c, grid);
    if (rc) return rc;
    if (kind == RIMPHONY_TABULATED) rim_tab_launch_norm(c->tab_kind, grid, st, pp, n, d_norm, c->d_queue.p, c->d_spill.p);
    else rim_with_kind(kind, [&](auto K) {
        hipLaunchKernelGGL(norm_kernel<decltype(K)::value>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pp, n, d_norm, c->d_queue.p, c->d_spill.p);
    });
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

static const int NPARAMS[5] = { 4, 1, 5, 4, 1 };

extern "C" int rimphony_dist_nparams(int kind)
{
    if (kind < 0 || kind > RIMPHONY_TABULATED) return RIMPHONY_EINVAL;
    return NPARAMS[kind];
}

// The tabulated distribution needs the context's table set: without one every entry refuses the kind.
static int check_tables(const rimphony_ctx *c, int kind)
{
    return (kind == RIMPHONY_TABULATED && !c->d_tab.p) ? RIMPHONY_EINVAL : RIMPHONY_OK;
}

// The one way a table set comes into a context or leaves it.  `blob` is the set as the kernels read it (tab_spline.h), of the
// form `tab_kind` (a DIST_TABULATED* value); an empty blob clears.  `fill`, if any, completes the set on the device, one wave
// per table: the tables' normalisations of a 2-D set (rim_tab_launch_table_norms), or P of the tables of a set with a sin^k
// prefactor and pitch rows (rim_tab_launch_pitchy_p), whose header is `fill_at` doubles into the set.  The new set is
// complete on the device before the previous one is let go: a refusal or a failed allocation leaves the previous set in
// place, and for the length of the call both are resident.
//
// With `dev`, `blob` is only the front of a 2-D set -- everything before its node data -- and the node data are solved on the
// device from dev->d_log_n (rimphony_tab_install.hip), on dev->st, the stream that produced them; the whole install runs on
// that stream.  This is the one path that sees values the host has not seen: a kernel looks for a non-finite one first, and
// such a set is refused (RIMPHONY_EINVAL) like any other, before anything is built.
typedef void (*RimTabFill)(unsigned grid, hipStream_t st, double *d_set, double *spill);
struct RimTabDeviceNodes {
    const double *d_log_n;
    size_t n_tables, n_nodes, n_mu;
    std::vector<double> axes;       // the axis block along u, then the one along mu (tab_install.h: rim_tab_install_axis)
    double hu, hmu;
    int grid_u, grid_mu;
    int ends_u, ends_mu;            // tab_spline.h: RIM_TAB_ENDS_*
    hipStream_t st;
};
static int install_tables(rimphony_ctx *c, const std::vector<double> &blob, int tab_kind, RimTabFill fill = nullptr, size_t fill_at = 0,
                          const RimTabDeviceNodes *dev = nullptr)
{
    const hipStream_t st = dev ? dev->st : nullptr;
    RimCtxScope scope(c, st);
    int rc = scope.enter();
    if (rc) return rc;
    // the previous set may still be read by the context's earlier work
    if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));
    if (blob.empty()) {
        c->d_tab.release();
        c->tab_kind = DIST_TABULATED_ISO;
        return RIMPHONY_OK;
    }
    const size_t node_doubles = dev ? dev->n_tables * dev->n_nodes * dev->n_mu * 4 : 0;
    const size_t total = blob.size() + node_doubles;
    RimDevBuf<double> fresh = { nullptr, 0 }, aux = { nullptr, 0 };
    if (dev) {
        // the axis blocks and, behind them, the word of the finiteness flag
        rc = aux.grow(dev->axes.size() + 1, (dev->axes.size() + 1) * sizeof(double), "the spline axes of the distribution tables");
        if (rc) return rc;
        unsigned *d_flag = (unsigned *) (aux.p + dev->axes.size()), bad = 0;
        hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(double), st);
        if (e == hipSuccess) {
            rim_tab_install_launch_finite(st, dev->d_log_n, node_doubles / 4, d_flag);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_flag, sizeof bad, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            rim_set_last_error("checking the distribution tables", hipGetErrorString(e));
            aux.release();
            return RIMPHONY_EHIP;
        }
        if (bad) { aux.release(); return RIMPHONY_EINVAL; }
    }
    rc = fresh.grow(total, total * sizeof(double), "the distribution tables");
    if (rc) { aux.release(); return rc; }
    const unsigned grid = persistent_grid(c, (unsigned long long) blob[TAB_HDR_NTABLES], 16);
    rc = ensure_spill(c, grid);
    if (rc) { fresh.release(); aux.release(); return rc; }
    hipError_t e;
    if (dev) {
        e = hipMemcpyAsync(fresh.p, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(aux.p, dev->axes.data(), dev->axes.size() * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            RimTabInstall s;
            s.log_n = dev->d_log_n;
            s.nodes = fresh.p + blob.size();
            s.n_tables = dev->n_tables; s.n_nodes = dev->n_nodes; s.n_mu = dev->n_mu;
            s.au = rim_tab_axis_of(aux.p, dev->n_nodes, dev->hu, dev->grid_u, dev->ends_u);
            s.amu = rim_tab_axis_of(aux.p + rim_tab_axis_doubles(dev->n_nodes), dev->n_mu, dev->hmu, dev->grid_mu, dev->ends_mu);
            rim_tab_install_launch_sweeps(st, s);
            e = hipGetLastError();
        }
    } else {
        e = hipMemcpy(fresh.p, blob.data(), blob.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && fill) {
        fill(grid, st, fresh.p + fill_at, c->d_spill.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    aux.release();
    if (e != hipSuccess) {
        rim_set_last_error("installing the distribution tables", hipGetErrorString(e));
        fresh.release();
        return RIMPHONY_EHIP;
    }
    c->d_tab.release();
    c->d_tab = fresh;
    c->tab_kind = tab_kind;
    return RIMPHONY_OK;
}

// The entries: check, build, install; n_tables = 0 clears through any of them.  A set of energy tables, each with a
// pitch row (log_g) or none with one (log_g null and n_mu = 0: the isotropic form).
extern "C" int rimphony_ctx_set_tables_pitch(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                             const double *log_n, size_t n_mu, const double *log_g)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_pitch(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g)) return RIMPHONY_EINVAL;
        try { rim_tab_build_pitch(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, log_g ? DIST_TABULATED : DIST_TABULATED_ISO);
}

extern "C" int rimphony_ctx_set_tables(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                       const double *log_n)
{
    return rimphony_ctx_set_tables_pitch(c, n_tables, n_nodes, gamma_lo, gamma_hi, log_n, 0, nullptr);
}

// A 2-D set: ln n(gamma, mu) on a grid.  The normalisation of each table is integrated once, as the set comes in
// (rimphony_tab.hip), and kept in the table's header, where the rows of a batch read it.
extern "C" int rimphony_ctx_set_tables_2d(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                          size_t n_mu, const double *log_n)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_2D, rim_tab_launch_table_norms);
}

// A 2-D set with a sin^k xi prefactor per table (sin_k null: the entry above).  k travels in the table's header; the
// normalisation, with the factor under the integral, is integrated as the set comes in (rimphony_tab_2d_pitchy.hip).
extern "C" int rimphony_ctx_set_tables_2d_pitchy(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                                 size_t n_mu, const double *log_n, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    if (!sin_k) return rimphony_ctx_set_tables_2d(c, n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n);
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_pitchy(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_pitchy(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_2D_PITCHY, rim_tab_2d_pitchy_launch_table_norms);
}

// A set with a sin^k xi prefactor per table (sin_k null: the entry above it).  Without g, P is the closed form
// rim_tab_build_pitchy set on the host; with g it is integrated once, as the set comes in, into the table's header, where
// norm_kernel reads it.
extern "C" int rimphony_ctx_set_tables_pitchy(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                              const double *log_n, size_t n_mu, const double *log_g, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    if (!sin_k) return rimphony_ctx_set_tables_pitch(c, n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g);
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_pitchy(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_pitchy(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_PITCHY, log_g ? rim_tab_launch_pitchy_p : nullptr);
}

// A family of energy tables: a row of a batch names a real index x in [0, n_tables - 1] and its samples blend tables floor(x)
// and floor(x) + 1 (rimphony_tab_family.hip; with sin_k rimphony_tab_family_pitchy.hip).  The plain forms' own checks and their
// own spline solve, table by table; nothing is integrated at install: the normalisation is per row.
extern "C" int rimphony_ctx_set_tables_family(rimphony_ctx *c, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                              const double *log_n, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_family(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_family(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, sin_k ? DIST_TABULATED_FAMILY_PITCHY : DIST_TABULATED_FAMILY);
}

// A family of 2-D surfaces on given gamma and mu nodes: a row of a batch names a real index x in [0, n_tables - 1] and its
// samples blend the node words of tables floor(x) and floor(x) + 1 (rimphony_tab_2d_family.hip; with sin_k
// rimphony_tab_2d_family_pitchy.hip).  The plain form's own check and its own solve; nothing is integrated at install.
extern "C" int rimphony_ctx_set_tables_2d_family(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                                 const double *mu, const double *log_n, const double *sin_k, int ends_gamma,
                                                 int ends_mu)
{
    if (!c || rim_tab_check_ends(ends_gamma, ends_mu)) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_family(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_family(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob, ends_gamma, ends_mu); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, sin_k ? DIST_TABULATED_2D_FAMILY_PITCHY : DIST_TABULATED_2D_FAMILY);
}

// The same family blended CUBICALLY across its tables: the set above followed by one knot word per table, `param` or 0, 1, 2 ..
// A sample blends the node words of four neighbouring tables with the Lagrange weights of its row
// (rimphony_tab_2d_family_cubic.hip; with sin_k rimphony_tab_2d_family_cubic_pitchy.hip).  The linear family's check and, on
// top of it, at least four tables and finite, strictly monotonic knots.
extern "C" int rimphony_ctx_set_tables_2d_family_cubic(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                                       const double *mu, const double *log_n, const double *sin_k, int ends_gamma,
                                                       int ends_mu, const double *param)
{
    if (!c || rim_tab_check_ends(ends_gamma, ends_mu)) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_family_cubic(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, param)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_family_cubic(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, param, blob, ends_gamma, ends_mu); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, sin_k ? DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY : DIST_TABULATED_2D_FAMILY_CUBIC);
}

// A set on gamma nodes of its own, always this form: the sin^k form's contents on the given nodes.  The host solves the
// spline and fills the guide (tab_spline.h: rim_tab_build_grid); where there are pitch rows, P is integrated by the sin^k
// form's kernel, which reads the tail of the set as a set of its own.
extern "C" int rimphony_ctx_set_tables_grid(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n,
                                            size_t n_mu, const double *log_g, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_grid(n_tables, n_nodes, gamma, log_n, n_mu, log_g, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_grid(n_tables, n_nodes, gamma, log_n, n_mu, log_g, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_GRID, log_g ? rim_tab_launch_pitchy_p : nullptr,
                          n_tables ? tab_grid_tail(n_tables, n_nodes, (size_t) blob[TAB_HDR_H]) : 0);
}

// A 2-D set on gamma nodes of its own: the 2-D form's surface on the given-nodes form's lookup (tab_spline.h:
// rim_tab_build_2d_grid).  The normalisation of each table is integrated once, as the set comes in (rimphony_tab_2d_grid.hip),
// into the word of the table's header where the rows of a batch read it.
extern "C" int rimphony_ctx_set_tables_2d_grid(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                               const double *log_n)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_2D_GRID, rim_tab_2d_grid_launch_table_norms);
}

// The same with a sin^k xi prefactor per table (sin_k null: the entry above), as rimphony_ctx_set_tables_2d_pitchy
// (rimphony_tab_2d_grid_pitchy.hip).
extern "C" int rimphony_ctx_set_tables_2d_grid_pitchy(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma,
                                                      size_t n_mu, const double *log_n, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    if (!sin_k) return rimphony_ctx_set_tables_2d_grid(c, n_tables, n_nodes, gamma, n_mu, log_n);
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_grid_pitchy(n_tables, n_nodes, gamma, n_mu, log_n, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_grid_pitchy(n_tables, n_nodes, gamma, n_mu, log_n, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    return install_tables(c, blob, DIST_TABULATED_2D_GRID_PITCHY, rim_tab_2d_grid_pitchy_launch_table_norms);
}

// A 2-D set on gamma nodes and mu nodes of the caller's choosing, with a sin^k xi prefactor per table or (sin_k null) without:
// the gamma lookup of the form above and the same kind of lookup along mu (rimphony_tab_2d_nodes.hip,
// rimphony_tab_2d_nodes_pitchy.hip).
extern "C" int rimphony_ctx_set_tables_2d_nodes(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                                const double *mu, const double *log_n, const double *sin_k)
{
    if (!c) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (n_tables) {
        if (rim_tab_check_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k)) return RIMPHONY_EINVAL;
        try { rim_tab_build_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob); }
        catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    }
    if (sin_k) return install_tables(c, blob, DIST_TABULATED_2D_NODES_PITCHY, rim_tab_2d_nodes_pitchy_launch_table_norms);
    return install_tables(c, blob, DIST_TABULATED_2D_NODES, rim_tab_2d_nodes_launch_table_norms);
}

// 0 where [p, p + bytes) is device memory of `device` as the runtime knows it.  An error the queries leave behind is cleared:
// it is this answer, not a failure of the install that follows.
static int check_device_range(const void *p, size_t bytes, int device)
{
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof attr);
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void) hipGetLastError(); return -1; }
    if (attr.type != hipMemoryTypeDevice || attr.device != device) return -1;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) p) != hipSuccess) { (void) hipGetLastError(); return -1; }
    const size_t off = (size_t) ((const char *) p - (const char *) base);
    return (off <= size && bytes <= size - off) ? 0 : -1;
}

// Any of the six 2-D forms from ln n in device memory: gamma null, the nodes uniform in ln gamma; mu null, uniform in mu;
// sin_k null, no prefactor.  The front of the set -- headers, guides, node words -- is the host entry's own
// (tab_spline.h: rim_tab_front_2d*); the node data are solved on the device (install_tables), to the host entry's bits.
// ends_u, ends_mu: the ends of the spline along u and along mu (tab_spline.h: RIM_TAB_ENDS_*), which the caller has checked.
static int set_tables_2d_device(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo, double gamma_hi,
                                size_t n_mu, const double *mu, const double *d_log_n, const double *sin_k, int ends_u, int ends_mu,
                                void *stream)
{
    if (!c) return RIMPHONY_EINVAL;
    const int ends = ends_u + 2 * ends_mu;
    std::vector<double> blob;
    if (!n_tables) return install_tables(c, blob, DIST_TABULATED_ISO);
    if (!gamma && mu) return RIMPHONY_EINVAL;
    if (!d_log_n) return RIMPHONY_EINVAL;
    if (mu ? rim_tab_check_2d_nodes_geometry(n_tables, n_nodes, gamma, n_mu, mu, sin_k)
           : gamma ? rim_tab_check_2d_grid_geometry(n_tables, n_nodes, gamma, n_mu)
                   : rim_tab_check_2d_geometry(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu))
        return RIMPHONY_EINVAL;
    if (sin_k && rim_tab_check_sin_k(n_tables, sin_k)) return RIMPHONY_EINVAL;
    if (check_device_range(d_log_n, n_tables * n_nodes * n_mu * sizeof(double), c->device)) return RIMPHONY_EINVAL;
    RimTabDeviceNodes dev;
    dev.d_log_n = d_log_n;
    dev.n_tables = n_tables; dev.n_nodes = n_nodes; dev.n_mu = n_mu;
    dev.hu = 0.; dev.hmu = 0.;
    dev.grid_u = gamma != nullptr; dev.grid_mu = mu != nullptr;
    dev.ends_u = ends_u; dev.ends_mu = ends_mu;
    dev.st = (hipStream_t) stream;
    int tab_kind;
    RimTabFill fill;
    try {
        std::vector<double> h, ih, hm, ihm;
        if (mu) {
            rim_tab_front_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, sin_k, blob, h, ih, hm, ihm, ends);
            tab_kind = sin_k ? DIST_TABULATED_2D_NODES_PITCHY : DIST_TABULATED_2D_NODES;
            fill = sin_k ? rim_tab_2d_nodes_pitchy_launch_table_norms : rim_tab_2d_nodes_launch_table_norms;
        } else if (gamma) {
            rim_tab_front_2d_grid(n_tables, n_nodes, gamma, n_mu, blob, h, ih, dev.hmu, ends);
            tab_kind = sin_k ? DIST_TABULATED_2D_GRID_PITCHY : DIST_TABULATED_2D_GRID;
            fill = sin_k ? rim_tab_2d_grid_pitchy_launch_table_norms : rim_tab_2d_grid_launch_table_norms;
        } else {
            rim_tab_front_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, blob, dev.hu, dev.hmu, ends);
            tab_kind = sin_k ? DIST_TABULATED_2D_PITCHY : DIST_TABULATED_2D;
            fill = sin_k ? rim_tab_2d_pitchy_launch_table_norms : rim_tab_launch_table_norms;
        }
        if (sin_k && !mu) rim_tab_put_2d_sin_k(n_tables, sin_k, blob);
        dev.axes.assign(rim_tab_axis_doubles(n_nodes) + rim_tab_axis_doubles(n_mu), 0.);
        rim_tab_install_axis(n_nodes, dev.hu, gamma ? h.data() : nullptr, gamma ? ih.data() : nullptr, dev.axes.data(), ends_u);
        rim_tab_install_axis(n_mu, dev.hmu, mu ? hm.data() : nullptr, mu ? ihm.data() : nullptr,
                             dev.axes.data() + rim_tab_axis_doubles(n_nodes), ends_mu);
    } catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    return install_tables(c, blob, tab_kind, fill, 0, &dev);
}

extern "C" int rimphony_ctx_set_tables_2d_device(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo,
                                                 double gamma_hi, size_t n_mu, const double *mu, const double *d_log_n,
                                                 const double *sin_k, void *stream)
{
    return set_tables_2d_device(c, n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, d_log_n, sin_k, RIM_TAB_ENDS_NATURAL,
                                RIM_TAB_ENDS_NATURAL, stream);
}

// The same with a choice of the spline's ends per axis (tab_spline.h: RIM_TAB_ENDS_*; anything else is refused before the set
// is looked at).  Natural ends on both axes: the set of the entry above.
extern "C" int rimphony_ctx_set_tables_2d_device_ends(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma,
                                                      double gamma_lo, double gamma_hi, size_t n_mu, const double *mu,
                                                      const double *d_log_n, const double *sin_k, int ends_gamma, int ends_mu, void *stream)
{
    if (!c || rim_tab_check_ends(ends_gamma, ends_mu)) return RIMPHONY_EINVAL;
    return set_tables_2d_device(c, n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, d_log_n, sin_k, ends_gamma, ends_mu, stream);
}

// Any of the six 2-D forms from ln n in HOST memory with a choice of the spline's ends per axis: gamma, mu and sin_k null or
// given as for the device entry.  Each form is checked and built by what its own entry calls, so natural ends on both axes
// install that entry's set, and what it refuses is refused here.
extern "C" int rimphony_ctx_set_tables_2d_ends(rimphony_ctx *c, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo,
                                               double gamma_hi, size_t n_mu, const double *mu, const double *log_n, const double *sin_k,
                                               int ends_gamma, int ends_mu)
{
    if (!c || rim_tab_check_ends(ends_gamma, ends_mu)) return RIMPHONY_EINVAL;
    std::vector<double> blob;
    if (!n_tables) return install_tables(c, blob, DIST_TABULATED_ISO);
    if (!gamma && mu) return RIMPHONY_EINVAL;
    int tab_kind;
    RimTabFill fill;
    try {
        if (mu) {
            if (rim_tab_check_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k)) return RIMPHONY_EINVAL;
            rim_tab_build_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob, ends_gamma, ends_mu);
            tab_kind = sin_k ? DIST_TABULATED_2D_NODES_PITCHY : DIST_TABULATED_2D_NODES;
            fill = sin_k ? rim_tab_2d_nodes_pitchy_launch_table_norms : rim_tab_2d_nodes_launch_table_norms;
        } else if (gamma) {
            if (rim_tab_check_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n) || (sin_k && rim_tab_check_sin_k(n_tables, sin_k)))
                return RIMPHONY_EINVAL;
            if (sin_k) rim_tab_build_2d_grid_pitchy(n_tables, n_nodes, gamma, n_mu, log_n, sin_k, blob, ends_gamma, ends_mu);
            else rim_tab_build_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n, blob, ends_gamma, ends_mu);
            tab_kind = sin_k ? DIST_TABULATED_2D_GRID_PITCHY : DIST_TABULATED_2D_GRID;
            fill = sin_k ? rim_tab_2d_grid_pitchy_launch_table_norms : rim_tab_2d_grid_launch_table_norms;
        } else {
            if (rim_tab_check_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n) || (sin_k && rim_tab_check_sin_k(n_tables, sin_k)))
                return RIMPHONY_EINVAL;
            if (sin_k) rim_tab_build_2d_pitchy(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, sin_k, blob, ends_gamma, ends_mu);
            else rim_tab_build_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, blob, ends_gamma, ends_mu);
            tab_kind = sin_k ? DIST_TABULATED_2D_PITCHY : DIST_TABULATED_2D;
            fill = sin_k ? rim_tab_2d_pitchy_launch_table_norms : rim_tab_launch_table_norms;
        }
    } catch (const std::bad_alloc &) { return RIMPHONY_ENOMEM; }
    return install_tables(c, blob, tab_kind, fill);
}

// The installed set as the kernels read it, copied to the host (diagnostics and tests).  It holds offsets, never addresses,
// so two installs of the same numbers compare word for word.  *n_doubles: the size of the set, 0 for none; RIMPHONY_EINVAL
// where `cap` doubles at `out` cannot hold it.
extern "C" int rimphony_debug_tables(rimphony_ctx *c, double *out, size_t cap, size_t *n_doubles)
{
    if (!c || !n_doubles) return RIMPHONY_EINVAL;
    RimCtxScope scope(c, nullptr);
    int rc = scope.enter();
    if (rc) return rc;
    *n_doubles = c->d_tab.p ? c->d_tab.cap : 0;
    if (!*n_doubles) return RIMPHONY_OK;
    if (!out || cap < *n_doubles) return RIMPHONY_EINVAL;
    HIP_TRY(hipMemcpy(out, c->d_tab.p, *n_doubles * sizeof(double), hipMemcpyDeviceToHost));
    return RIMPHONY_OK;
}

static int rim_precision_check(const rimphony_ctx *c, int kind, int precision);

// The argument checks of the batch entries, in the order every entry applies them: the kind and the `head` pointers
// (RIMPHONY_EINVAL), the precision (prec_ctx != null; RIMPHONY_ENOTSUP), the empty batch (*empty set, RIMPHONY_OK: nothing
// to read or write), the `data` pointers and the kind's parameter arrays (params != null; RIMPHONY_EINVAL).  Which code an
// odd call gets depends on which pointers an entry puts before and which after the empty batch, so each entry says so.
static int check_batch_args(int kind, std::initializer_list<const void *> head, const rimphony_ctx *prec_ctx, int precision,
                            size_t n, bool *empty, std::initializer_list<const void *> data, const double *const *params)
{
    *empty = false;
    if (kind < 0 || kind > RIMPHONY_TABULATED) return RIMPHONY_EINVAL;
    for (const void *q : head) if (!q) return RIMPHONY_EINVAL;
    if (prec_ctx) { const int prc = rim_precision_check(prec_ctx, kind, precision); if (prc) return prc; }
    if (n == 0) { *empty = true; return RIMPHONY_OK; }
    for (const void *q : data) if (!q) return RIMPHONY_EINVAL;
    if (params)
        for (int k = 0; k < NPARAMS[kind]; k++) if (!params[k]) return RIMPHONY_EINVAL;
    return RIMPHONY_OK;
}

// The lines of `n` rows of a family with a sin^k prefactor or of a family of 2-D surfaces: room for them in the context, and
// their address in pp.p[2] (load_params), where the normalisation's launch writes them.  Any other set: nothing.
static_assert(TAB_FAMILY_LINE == TAB_2D_HDR, "one array serves the lines of either kind of family");
static bool tab_kind_has_lines(int tab_kind) { return tab_kind == DIST_TABULATED_FAMILY_PITCHY || tab_kind_2d_family(tab_kind); }
// (the line of a family of 2-D surfaces blended cubically is wider: load_params strides by the same rule)
static size_t tab_kind_line_doubles(int tab_kind) { return tab_kind_2d_family_cubic(tab_kind) ? TAB_2D_CUBIC_LINE : TAB_FAMILY_LINE; }
static int family_lines(rimphony_ctx *c, int kind, size_t n, ParamPtrs &pp)
{
    if (kind != RIMPHONY_TABULATED || !tab_kind_has_lines(c->tab_kind)) return RIMPHONY_OK;
    // (counted in doubles, not rows: the buffer outlives a change of form, and the forms' lines differ in width)
    const size_t doubles = n * tab_kind_line_doubles(c->tab_kind);
    const int rc = c->d_famline.grow(doubles, doubles * sizeof(double), "the rows' lines of a table family");
    if (rc) return rc;
    pp.p[2] = c->d_famline.p;
    return RIMPHONY_OK;
}

static int make_param_ptrs(const rimphony_ctx *c, int kind, const double *const *d_params, ParamPtrs &pp)
{
    bool empty;
    int rc = check_batch_args(kind, { d_params }, nullptr, 0, 1, &empty, {}, d_params);
    if (!rc) rc = check_tables(c, kind);
    if (rc) return rc;
    for (int k = 0; k < 5; k++) pp.p[k] = k < NPARAMS[kind] ? d_params[k] : nullptr;
    if (kind == RIMPHONY_TABULATED) pp.p[1] = c->d_tab.p;       // (load_params: the kind's p[1] is the table set)
    return RIMPHONY_OK;
}

extern "C" int rimphony_batch_norm_device(rimphony_ctx *c, int kind, size_t n, const double *const *d_params,
                                          double *d_norm, void *stream)
{
    bool empty;
    int rc = check_batch_args(kind, { c }, nullptr, 0, n, &empty, { d_norm, d_params }, d_params);
    if (!rc) rc = check_tables(c, kind);
    if (rc || empty) return rc;
    hipStream_t st = (hipStream_t) stream;
    RimCtxScope scope(c, st);
    rc = scope.enter();
    if (rc) return rc;
    ParamPtrs pp;
    rc = make_param_ptrs(c, kind, d_params, pp);
    if (!rc) rc = family_lines(c, kind, n, pp);
    if (rc) return rc;
    return launch_norm(c, kind, n, pp, d_norm, st);
}

// ---- the persistent launch ----------------------------------------------------------------------------------------
// What differs between the kernels that run as a persistent grid with a cooperative tail: coop_kernel<P> (one wave per
// coefficient) and group_kernel<P> (group_kernel.h: the coefficients of a point in lock-step).
struct PersistentKernel {
    const void *fn;                 // kernel entry: occupancy and attribute queries, launch
    int waves;                      // waves per SIMD of its launch bounds
    bool early_help;                // it has the early-help protocol (coop_common.h) ...
    unsigned early_squad;           // ... with this default squad
    bool faraday;                   // which pair of timing events brackets it
    int *resident;                  // the context's cache cell for the occupancy answer
    RimDevBuf<double> *spill;       // per-wave spill region and
    size_t spill_doubles;           // ... its doubles per wave
    RimDevBuf<char> *board;         // the board,
    size_t slot_bytes;              // ... the size of a slot
    size_t clear_bytes;             // ... and how much of a slot is zeroed before a launch
    const char *launch_what;        // names a failed launch in the error text
};

// coop_kernel<P> of a problem (0: Symphony, prec 1: its fp32-integrand variant; 1: Heyvaerts) and distribution kind
template <class P>
static PersistentKernel coop_kernel_of()
{
    PersistentKernel k = {};
    k.fn = reinterpret_cast<const void *>(coop_kernel<P>);
    k.waves = (int) P::WAVES;
    k.early_help = P::EARLY_HELP != 0;
    k.early_squad = (unsigned) P::EARLY_SQUAD;
    return k;
}
static PersistentKernel rim_coop_kernel(int problem, int kind, int prec, int tab_kind)
{
    if (kind == RIMPHONY_TABULATED) {       // (its kernels live in rimphony_tab.hip; no fp32 variant: refused at the entry)
        const RimCoopKernelInfo t = rim_tab_coop_kernel(problem, tab_kind);
        PersistentKernel k = {};
        k.fn = t.fn; k.waves = t.waves; k.early_help = t.early_help; k.early_squad = t.early_squad;
        return k;
    }
    return rim_with_kind(kind, [&](auto K) -> PersistentKernel {
        constexpr int KIND = decltype(K)::value;
        if (problem) return coop_kernel_of<HeyvaertsProblem<KIND>>();
        if (!prec) return coop_kernel_of<SymphonyProblem<KIND>>();
#if defined(RIM_F32_SMOOTH)
        constexpr int F32_KIND = KIND;                  // the measurement build of the "smooth" variant serves all four kinds
#else
        constexpr int F32_KIND = KIND == 0 ? 0 : 1;     // (kinds 2 and 3 were refused at the entry: RIMPHONY_ENOTSUP)
#endif
        return coop_kernel_of<SymphonyProblem<F32_KIND, 1>>();
    });
}

// Plans the grid, grows the spill region and the board, lets `fill(plan)` complete the kernel's argument struct (`base` is
// the SymArgs inside it, `kargs` the struct itself) and enqueues: board clear, board_init_kernel, start event, kernel, stop
// event.
template <class Fill>
static int launch_persistent(rimphony_ctx *c, const PersistentKernel &k, unsigned long long ntasks, SymArgs &base, void *kargs,
                             hipStream_t st, Fill &&fill)
{
    // how many of these workgroups a CU holds (launch_plan.h): asked once per context and instantiation
    if (*k.resident == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k.fn, 64, RIM_DYN_LDS) != hipSuccess || nb < 1) nb = -1;
        *k.resident = nb;
    }
    size_t static_lds = 0, dyn_lds = 0;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, k.fn) == hipSuccess) { static_lds = fa.sharedSizeBytes; dyn_lds = RIM_DYN_LDS; }
    const unsigned want_squad = c->knobs.early_squad >= 0 ? (unsigned) c->knobs.early_squad : k.early_squad;
    const RimGridPlan plan = rim_plan_grid(c->n_cu, ntasks, *k.resident, static_lds, dyn_lds, k.waves, c->shared_mode != 0,
                                           c->no_assist != 0, want_squad, k.early_help);
    const unsigned grid = plan.grid;
    // The group kernels' region holds, per wave, four members' lists at the GSL limits of the path -- 0.86 MB for the
    // Symphony groups (5000 + 1000 entries), 1.3 MB for the Faraday pair in lock-step (4096 + 4096; off by default): 4.4 GB
    // of the 288 for a full persistent grid of 5120 waves, held until the context is destroyed.  One sized for the Symphony
    // groups does not serve the Faraday pair.
    const bool group = k.spill == &c->d_gspill;
    if (group && k.faraday && !c->gspill_faraday) c->d_gspill.release();
    if (k.spill->cap < grid) {
        char what[160];
        snprintf(what, sizeof what, "the subinterval spill region of %u waves (lists beyond the LDS part)", grid);
        const int rc = k.spill->grow(grid, (size_t) grid * k.spill_doubles * sizeof(double), what);
        if (rc) return rc;
        if (group) c->gspill_faraday = k.faraday;
    }
    int rc = k.board->grow(grid, (size_t) grid * k.slot_bytes + BOARD_FLAG_WORDS * sizeof(unsigned), "the board of the cooperative tail");
    if (rc) return rc;
    base.board_flags = (unsigned *) (k.board->p + k.board->cap * k.slot_bytes);
    base.idle_ticks = 2ull * c->ticks_per_s;
    base.owner_ticks = c->owner_wait_ticks;
    rc = fill(plan);
    if (rc) return rc;
    // every claim word starts closed (count 0; the payload arrays of a GroupSlot need no reset: an entry is written before
    // its round is opened); flags: not exhausted, the waves that may fetch a task (the squad never does), nobody idle
    if (k.clear_bytes == k.slot_bytes) HIP_TRY(hipMemsetAsync(k.board->p, 0, (size_t) grid * k.slot_bytes, st));
    else HIP_TRY(hipMemset2DAsync(k.board->p, k.slot_bytes, 0, k.clear_bytes, grid, st));
    hipLaunchKernelGGL(board_init_kernel, dim3(1), dim3(128), RIM_DYN_LDS, st, base.board_flags, grid - plan.early_squad);
    HIP_TRY(hipEventRecord(k.faraday ? c->ev_fstart : c->ev_start, st));
    void *params[] = { kargs };
    hipError_t e = hipLaunchKernel(k.fn, dim3(grid), dim3(64), params, RIM_DYN_LDS, st);
    const hipError_t last = hipGetLastError();
    if (e == hipSuccess) e = last;
    if (e != hipSuccess) {
        rim_set_last_error(k.launch_what, hipGetErrorString(e));
        return RIMPHONY_EHIP;
    }
    HIP_TRY(hipEventRecord(k.faraday ? c->ev_fstop : c->ev_stop, st));
    if (k.faraday) c->evf_valid = 1; else c->ev_valid = 1;
    return RIMPHONY_OK;
}

// One wave per (point, coefficient): coop_kernel<SymphonyProblem> (problem 0) or coop_kernel<HeyvaertsProblem> (1).
static int launch_coop(rimphony_ctx *c, int problem, int kind, int prec, const SymArgs &a, hipStream_t st)
{
    PersistentKernel k = rim_coop_kernel(problem, kind, prec, c->tab_kind);
    k.faraday = problem != 0;
    k.resident = prec ? &c->resident_f32[kind] : &c->resident[problem][kind != RIMPHONY_TABULATED ? kind : c->tab_kind];
    k.spill = &c->d_spill;
    k.spill_doubles = SPILL_DOUBLES_PER_WAVE;
    k.board = &c->d_board;
    k.slot_bytes = k.clear_bytes = sizeof(AssistSlot);
    k.launch_what = "hipGetLastError()";
    SymArgs b = a;
    return launch_persistent(c, k, (unsigned long long) a.n * (unsigned) a.nslots, b, &b, st, [&](const RimGridPlan &plan) -> int {
        b.spill = c->d_spill.p;
        b.board = c->no_assist ? nullptr : (AssistSlot *) c->d_board.p;
        b.early_squad = plan.early_squad;
        b.early_stride = plan.early_stride;
        b.early_classes = plan.early_classes;
        b.early_min = (int) c->knobs.early_min;
        b.turbo = (int) c->knobs.rounds;
        return RIMPHONY_OK;
    });
}

// The slots of a batch as (point, group) tasks (group_kernel.h).  Symphony: group 0 = the selected ones of
// {j_I, alpha_I, j_Q, alpha_Q}, group 1 = those of {j_V, alpha_V} (symphony_group.h); Faraday: the one group
// {rho_Q, rho_V} (heyvaerts_group.h).
static int launch_group(rimphony_ctx *c, int kind, const SymArgs &a, uint32_t coeff_mask, int faraday, hipStream_t st)
{
    GroupArgs ga = {};
    ga.base = a;
    for (int grp = 0; grp < (faraday ? 1 : 2); grp++) {
        unsigned packed = 0;
        int nm = 0;
        const int lo = faraday ? 6 : (grp ? 4 : 0), hi = faraday ? 8 : (grp ? 6 : 4);
        for (int k = lo; k < hi; k++)
            if (coeff_mask & (1u << k)) { packed |= (unsigned) k << (4 * nm); nm++; }
        if (nm) { ga.gslots[ga.ngroups] = packed; ga.gnmem[ga.ngroups] = nm; ga.ngroups++; }
    }
    if (ga.ngroups == 0) return RIMPHONY_OK;
    PersistentKernel k = {};
    // (the tabulated kind: one instantiation and one cell per form of the installed set, as in launch_coop; Symphony groups only)
    const bool tab = kind == RIMPHONY_TABULATED;
    if (tab && faraday) return RIMPHONY_ENOTSUP;
    k.fn = tab ? rim_tab_group_kernel(c->tab_kind) : rim_group_kernel(kind, faraday);
    k.waves = rim_group_waves(faraday);
    k.faraday = faraday != 0;
    k.resident = &c->resident_group[faraday ? 1 : 0][tab ? c->tab_kind : kind];
    k.spill = &c->d_gspill;
    // (never less than the Symphony groups' size)
    k.spill_doubles = faraday && SPILL_HEYGROUP_DOUBLES_PER_WAVE > SPILL_GROUP_DOUBLES_PER_WAVE ? SPILL_HEYGROUP_DOUBLES_PER_WAVE
                                                                                                : SPILL_GROUP_DOUBLES_PER_WAVE;
    k.board = &c->d_gboard;
    k.slot_bytes = sizeof(GroupSlot);
    k.clear_bytes = 32;             // claim, point, done, slots
    k.launch_what = "group_kernel launch";
    return launch_persistent(c, k, (unsigned long long) a.n * (unsigned) ga.ngroups, ga.base, &ga, st, [&](const RimGridPlan &plan) -> int {
        ga.gspill = c->d_gspill.p;
        ga.gboard = (GroupSlot *) c->d_gboard.p;
        ga.coop = c->no_assist ? 0 : 1;
        ga.base.board = nullptr;
#if defined(RIM_PROF)
        if (plan.grid <= RIM_PROF_ROWS) HIP_TRY(hipGetSymbolAddress((void **) &ga.prof, HIP_SYMBOL(g_rim_prof)));
#endif
        (void) plan;
        return RIMPHONY_OK;
    });
}

// Where the Symphony slots of the tabulated distribution run when RIMPHONY_TAB_GROUP does not say: on the group kernel or
// one wave per coefficient, per form of the installed set; a 2-D set on given nodes (DIST_TABULATED_2D_GRID) has no line of
// its own and takes the 2-D form's, as do the 2-D forms with a sin^k prefactor and those on given mu nodes.  NOT MEASURED yet: every form says "group" until the file its line names has figures --
// profiles/tabulated_group_times.txt, profiles/tabulated_grid_times.txt for a set on given gamma nodes.
static const bool RIM_TAB_GROUP_DEFAULT[5] = {      // [tab_kind - DIST_TABULATED]
    true,       // DIST_TABULATED, pitch rows   NOT MEASURED (profiles/tabulated_group_times.txt)
    true,       // DIST_TABULATED_ISO           NOT MEASURED (profiles/tabulated_group_times.txt)
    true,       // DIST_TABULATED_2D            NOT MEASURED (profiles/tabulated_group_times.txt)
    true,       // DIST_TABULATED_PITCHY        NOT MEASURED (profiles/tabulated_group_times.txt)
    true,       // DIST_TABULATED_GRID          NOT MEASURED (profiles/tabulated_grid_times.txt)
};
// (A family of energy tables has no line of its own either: it takes the line of the plain form its integer rows are -- the
// isotropic form's, or with a prefactor the sin^k form's -- until profiles/tabulated_family_times.txt says otherwise.  A family
// of 2-D surfaces takes the 2-D form's, as every 2-D form does; measured for it, the group kernel is 1.5 x (no prefactor) and
// 2.0 x (sin^k) faster per Symphony sample than one wave per coefficient: profiles/tabulated_2d_family_times.txt.  The same
// family blended cubically takes the same line: profiles/tabulated_2d_family_cubic_times.txt.)
static bool rim_tab_runs_group(const rimphony_ctx *c)
{
    if (c->knobs.tab_group >= 0) return c->knobs.tab_group != 0;
    const int form = c->tab_kind == DIST_TABULATED_FAMILY ? (int) DIST_TABULATED_ISO
                   : c->tab_kind == DIST_TABULATED_FAMILY_PITCHY ? (int) DIST_TABULATED_PITCHY
                   : c->tab_kind >= DIST_TABULATED_2D_GRID ? (int) DIST_TABULATED_2D : c->tab_kind;
    return RIM_TAB_GROUP_DEFAULT[form - DIST_TABULATED];
}

// `precision` of the batch entries.  F64 is the product.  F32_INTEGRAND (BASELINE configs[4]'s fp32-core integrand) is
// NOT offered: on the anisotropic distributions -- pitchy kappa is the one configs[4] names -- its 1e-7 non-smooth noise
// sits above GSL's round-off detectors on integrals that cancel (1.53 x slower than fp64, 1.9 % new NaNs, round 2); on the
// power-law and thermal distributions it ran 0.90 / 0.96 of the fp64 time of the ROUND-2 kernel it is built on, and the
// fp64 default has since moved to the group kernel at 0.66 of that time: the variant is 1.36-1.43 x SLOWER than fp64 and
// lossier.  A precision that is slower and lossier is not a mode, it is a trap: RIMPHONY_ENOTSUP for
// every kind, unless the context was created with RIMPHONY_F32_VARIANT=1 (measurement hook: tools/f32_variant.py, the
// error-envelope test), and even then not for the anisotropic kinds.
static int rim_precision_check(const rimphony_ctx *c, int kind, int precision)
{
    if (precision == RIMPHONY_PRECISION_F64) return RIMPHONY_OK;
    if (precision != RIMPHONY_PRECISION_F32_INTEGRAND || !c || !c->knobs.f32_variant) return RIMPHONY_ENOTSUP;
    if (kind == RIMPHONY_TABULATED) return RIMPHONY_ENOTSUP;
#if !defined(RIM_F32_SMOOTH)      // (the measurement build of the "smooth" variant serves all four kinds)
    if (kind == RIMPHONY_PITCHY_PL || kind == RIMPHONY_PITCHY_KAPPA) return RIMPHONY_ENOTSUP;
#endif
    return RIMPHONY_OK;
}

// The batch entry points share the context's workspace (task queue, norms, visiting order, spill regions, assist
// board, timing events).  Calls on one context are therefore serialised on the host (c->mu) and ordered on the device:
// a call's stream first waits for the event the previous call recorded after its last kernel, whatever stream that was.
static int batch_compute_locked(rimphony_ctx *c, int kind, size_t n, const double *d_s, const double *d_theta,
                                const double *const *d_params, uint32_t coeff_mask, int precision,
                                double *d_out, int32_t *d_status, uint64_t *d_work, hipStream_t st);

extern "C" int rimphony_batch_compute_device_ex(rimphony_ctx *c, int kind, size_t n,
                                                const double *d_s, const double *d_theta,
                                                const double *const *d_params, uint32_t coeff_mask, int precision,
                                                double *d_out, int32_t *d_status, uint64_t *d_work, void *stream)
{
    bool empty;
    int rc = check_batch_args(kind, { c }, c, precision, n, &empty, { d_out, d_s, d_theta }, nullptr);
    if (!rc) rc = check_tables(c, kind);
    if (rc || empty) return rc;
    hipStream_t st = (hipStream_t) stream;
    RimCtxScope scope(c, st);
    rc = scope.enter();
    if (rc) return rc;
    return batch_compute_locked(c, kind, n, d_s, d_theta, d_params, coeff_mask, precision, d_out, d_status, d_work, st);
}

extern "C" int rimphony_batch_compute_device(rimphony_ctx *c, int kind, size_t n,
                                             const double *d_s, const double *d_theta,
                                             const double *const *d_params, uint32_t coeff_mask,
                                             double *d_out, int32_t *d_status, void *stream)
{
    return rimphony_batch_compute_device_ex(c, kind, n, d_s, d_theta, d_params, coeff_mask, RIMPHONY_PRECISION_F64,
                                            d_out, d_status, nullptr, stream);
}

static int batch_compute_locked(rimphony_ctx *c, int kind, size_t n, const double *d_s, const double *d_theta,
                                const double *const *d_params, uint32_t coeff_mask, int precision,
                                double *d_out, int32_t *d_status, uint64_t *d_work, hipStream_t st)
{
    ParamPtrs pp;
    int rc = make_param_ptrs(c, kind, d_params, pp);
    if (rc) return rc;

    rc = ensure_norm(c, n);
    if (!rc) rc = family_lines(c, kind, n, pp);
    if (rc) return rc;

    // full_calculation()
    rc = launch_norm(c, kind, n, pp, c->d_norm.p, st);
    if (rc) return rc;

    // what both launches share; the launch itself sets what it decides (launch_persistent)
    SymArgs base = {};
    base.early_stride = 1;
    base.early_classes = 1;
    base.pp = pp;
    base.s = d_s;
    base.theta = d_theta;
    base.norm = c->d_norm.p;
    base.out = d_out;
    base.status = d_status;
    base.n = n;
    base.queue = c->d_queue.p;
    base.heartbeat = c->hb_dev;
    base.hb_task = c->hb_task;
    base.work = (unsigned long long *) d_work;
    const bool ordered = n > 4096 && n < 0xffffffffull;
    const double *const order_gmin = (kind == RIMPHONY_POWER_LAW) ? pp.p[1] : (kind == RIMPHONY_PITCHY_PL) ? pp.p[2] : nullptr;
    const double *const order_temp = (kind == RIMPHONY_THERMAL_JUETTNER) ? pp.p[0] : nullptr;
    // the visiting order of the Symphony launch now; the Faraday launch gets its own (same array, rebuilt on the stream
    // after the Symphony kernel: see below)
    auto build_order = [&](int faraday) -> int {
        unsigned *hist = c->d_perm.p + c->d_perm.cap;
        const unsigned nb = (unsigned) ((n + 255) / 256);
        HIP_TRY(hipMemsetAsync(hist, 0, ORDER_BUCKETS * sizeof(unsigned), st));
        hipLaunchKernelGGL(order_hist_kernel, dim3(nb), dim3(256), RIM_DYN_LDS, st, d_s, d_theta, order_gmin, order_temp, n, hist, faraday);
        hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(64), RIM_DYN_LDS, st, hist);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(nb), dim3(256), RIM_DYN_LDS, st, d_s, d_theta, order_gmin, order_temp, n, hist,
                           c->d_perm.p, faraday);
        HIP_TRY(hipGetLastError());
        return RIMPHONY_OK;
    };
    if (ordered) {
        rc = build_order(0);
        if (rc) return rc;
        base.perm = c->d_perm.p;
    }
    if (d_work) HIP_TRY(hipMemsetAsync(d_work, 0, n * 8 * sizeof(uint64_t), st));
    SymArgs a = base, fa = base;
    uint32_t computed = 0;
    for (int k = 0; k < 6; k++)     // symphony slots: j/alpha x I,Q,V
        if (coeff_mask & (1u << k)) { a.slot[a.nslots++] = k; computed |= 1u << k; }
    for (int k = 6; k < 8; k++)     // Faraday slots: rho_Q, rho_V
        if (coeff_mask & (1u << k)) { fa.slot[fa.nslots++] = k; computed |= 1u << k; }

    HIP_TRY(hipMemsetAsync(c->d_queue.p, 0, 16 * sizeof(unsigned long long), st));
    {
        const size_t total = n * 8;
        hipLaunchKernelGGL(fill_unselected_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), RIM_DYN_LDS, st,
                           d_out, d_status, n, computed);
        HIP_TRY(hipGetLastError());
    }
    if (a.nslots > 0) {
        if (precision == RIMPHONY_PRECISION_F32_INTEGRAND) {
            // the six Symphony coefficients with the fp32-core integrand (detmath.h); the Faraday pair below stays fp64
            // (kinds 2 and 3 were refused at the entry: RIMPHONY_ENOTSUP)
            rc = launch_coop(c, 0, kind, 1, a, st);
        } else if (!c->knobs.sym_solo && (kind != RIMPHONY_TABULATED || rim_tab_runs_group(c))) {
            // the coefficients of a point that share their samples advance in lock-step on one wave
            rc = launch_group(c, kind, a, coeff_mask, 0, st);
            if (rc == RIMPHONY_ENOMEM && kind == RIMPHONY_TABULATED) {
                // no room for the group kernel's workspace (its spill region is 4.4 GB for a full grid, launch_persistent;
                // nothing has been enqueued): the batch runs where the kind ran before it had group kernels, same bits
                rim_clear_last_error();
                rc = launch_coop(c, 0, kind, 0, a, st);
            }
        } else {
            // (RIMPHONY_SYM_SOLO=1, or a form of the tabulated distribution whose Symphony slots are not on the group kernel)
            rc = launch_coop(c, 0, kind, 0, a, st);
        }
        if (rc) return rc;
    }
    if (fa.nslots > 0 && ordered && !c->knobs.faraday_symphony_order) {
        rc = build_order(1);
        if (rc) return rc;
    }
    if (fa.nslots > 0 && c->knobs.faraday_group && kind != RIMPHONY_TABULATED) {
        // rho_Q and rho_V of a point in lock-step (heyvaerts_group.h): they share their samples' coordinates, distribution
        // derivatives and Bessel functions.  Bit-identical, and measured SLOWER than one wave per coefficient (an executed
        // pass serves 1.38 coefficients and costs 1.6 solo passes: DESIGN.md section 5) -- off unless asked for.
        rc = launch_group(c, kind, fa, coeff_mask, 1, st);
        if (rc) return rc;
    } else if (fa.nslots > 0) {
        rc = launch_coop(c, 1, kind, 0, fa, st);
        if (rc) return rc;
    }
    return RIMPHONY_OK;
}

extern "C" int rimphony_debug_heartbeat(rimphony_ctx *c, uint64_t task, uint64_t **host_words)
{
    if (!c || !host_words) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (!c->hb_host) {
        void *h = nullptr, *d = nullptr;
        HIP_TRY(hipHostMalloc(&h, 16 * sizeof(unsigned long long), hipHostMallocMapped));
        memset(h, 0, 16 * sizeof(unsigned long long));
        HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
        c->hb_host = (unsigned long long *) h;
        c->hb_dev = (unsigned long long *) d;
    }
    // the group kernel (the default for the Symphony slots) writes no heartbeat: a watchdog polling word [10] would
    // wait for ever
    if (!(task & (1ull << 62)) && !c->knobs.sym_solo) {
        rim_set_last_error("rimphony_debug_heartbeat", "Symphony tasks are only watched with RIMPHONY_SYM_SOLO=1");
        return RIMPHONY_ENOTSUP;
    }
    c->hb_task = task;
    *host_words = (uint64_t *) c->hb_host;
    return RIMPHONY_OK;
}

extern "C" int rimphony_debug_counters(rimphony_ctx *c, uint64_t out[32])
{
    if (!c || !out) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
#if defined(RIM_PROF)
    {   // diagnostic build: 32 region timers summed over waves (then reset); out must hold 32 words
        static unsigned long long hostbuf[RIM_PROF_ROWS * 32];
        HIP_TRY(hipMemcpyFromSymbol(hostbuf, HIP_SYMBOL(g_rim_prof), sizeof hostbuf));
        for (int k = 0; k < 32; k++) out[k] = 0;
        for (size_t r = 0; r < RIM_PROF_ROWS; r++) for (int k = 0; k < 32; k++) out[k] += hostbuf[r * 32 + k];
        memset(hostbuf, 0, sizeof hostbuf);
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rim_prof), hostbuf, sizeof hostbuf));
        return RIMPHONY_OK;
    }
#endif
    for (int k = 16; k < 32; k++) out[k] = 0;
    if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));     // the launch may be on a non-blocking stream
    HIP_TRY(hipMemcpy(out, c->d_queue.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RIMPHONY_OK;
}

extern "C" int rimphony_last_symphony_ms(rimphony_ctx *c, float *ms)
{
    if (!c || !ms) return RIMPHONY_EINVAL;
    if (!c->ev_valid) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_stop));
    HIP_TRY(hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    return RIMPHONY_OK;
}

extern "C" int rimphony_last_faraday_ms(rimphony_ctx *c, float *ms)
{
    if (!c || !ms) return RIMPHONY_EINVAL;
    if (!c->evf_valid) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_fstop));
    HIP_TRY(hipEventElapsedTime(ms, c->ev_fstart, c->ev_fstop));
    return RIMPHONY_OK;
}

extern "C" int rimphony_last_work(rimphony_ctx *c, rimphony_work *out)
{
    if (!c || !out) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[8];
    if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));     // the launch may be on a non-blocking stream
    HIP_TRY(hipMemcpy(h, c->d_queue.p, sizeof h, hipMemcpyDeviceToHost));
    out->samples = h[1];
    out->passes = h[2];
    out->inner_qags = h[3];
    out->faraday_samples = h[5];
    out->faraday_passes = h[6];
    out->faraday_inner_qags = h[7];
    return RIMPHONY_OK;
}

extern "C" int rimphony_last_tail(rimphony_ctx *c, uint64_t out[8])
{
    if (!c || !out) return RIMPHONY_EINVAL;
    // the queue words belong to the context's workspace: read them under its lock, after the last call's kernels
    // (a concurrent call on the same context resets them)
    std::lock_guard<std::recursive_mutex> lock(*c->mu);
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h[16];
    if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));
    HIP_TRY(hipMemcpy(h, c->d_queue.p, sizeof h, hipMemcpyDeviceToHost));
    out[0] = h[14] >> 40; out[1] = h[14] & 0xffffffffffull;        // (batches << 40) | row: rows to 1.1e12
    out[2] = h[15] >> 40; out[3] = h[15] & 0xffffffffffull;
    out[4] = h[8]; out[5] = h[9];
    out[6] = h[10]; out[7] = h[11];
    return RIMPHONY_OK;
}

extern "C" int rimphony_batch_compute_ex(rimphony_ctx *c, int kind, size_t n,
                                         const double *s, const double *theta, const double *const *params,
                                         uint32_t coeff_mask, int precision, double *out, int32_t *status, uint64_t *work)
{
    bool empty;
    int rc0 = check_batch_args(kind, { c, out, params }, c, precision, n, &empty, { s, theta }, params);
    if (!rc0) rc0 = check_tables(c, kind);
    if (rc0 || empty) return rc0;
    const int np = NPARAMS[kind];
    // ONE lock across staging, launch, synchronisation and copy-out: the staging buffers belong to the context, and a
    // second thread on the same context must not overwrite or re-allocate them before this call has copied its
    // table out (include/rimphony_hip.h: "Calls on one context are serialised").  The device entry below re-locks
    // the same (recursive) mutex.
    RimCtxScope scope(c, nullptr);
    rim_clear_last_error();
    HIP_TRY(hipSetDevice(c->device));
    const double *dp[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    uint64_t *d_work = nullptr;
    {
        if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));   // the staging buffers may still be in use
        const size_t need_in = n * (size_t) (2 + np);
        int rcb = c->d_in.grow(need_in, need_in * sizeof(double), "the staged inputs");
        if (rcb) return rcb;
        if (c->d_out.cap < n) {
            // the pair grows together; status and the optional work counters share one allocation: [n][8] int32, then
            // [n][8] uint64
            c->d_status.release();
            rcb = c->d_out.grow(n, n * 8 * sizeof(double), "the staged table");
            if (!rcb) rcb = c->d_status.grow(n, n * 8 * (sizeof(int32_t) + sizeof(uint64_t)), "the staged status words and work counters");
            if (rcb) { c->d_out.release(); return rcb; }
        }
        HIP_TRY(hipMemcpy(c->d_in.p, s, n * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c->d_in.p + n, theta, n * sizeof(double), hipMemcpyHostToDevice));
        for (int k = 0; k < np; k++) {
            HIP_TRY(hipMemcpy(c->d_in.p + (size_t) (2 + k) * n, params[k], n * sizeof(double), hipMemcpyHostToDevice));
            dp[k] = c->d_in.p + (size_t) (2 + k) * n;
        }
        if (work) d_work = (uint64_t *) (c->d_status.p + c->d_status.cap * 8);
    }
    int rc = rimphony_batch_compute_device_ex(c, kind, n, c->d_in.p, c->d_in.p + n, dp, coeff_mask, precision, c->d_out.p,
                                              c->d_status.p, d_work, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out, c->d_out.p, n * 8 * sizeof(double), hipMemcpyDeviceToHost));
    if (status) HIP_TRY(hipMemcpy(status, c->d_status.p, n * 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (work) HIP_TRY(hipMemcpy(work, d_work, n * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RIMPHONY_OK;
}

extern "C" int rimphony_batch_compute(rimphony_ctx *c, int kind, size_t n,
                                      const double *s, const double *theta, const double *const *params,
                                      uint32_t coeff_mask, double *out, int32_t *status)
{
    return rimphony_batch_compute_ex(c, kind, n, s, theta, params, coeff_mask, RIMPHONY_PRECISION_F64, out, status, nullptr);
}

// ---- multi-device batch (SURVEY 8b `n_devices`, 8e) --------------------------------------------
// Row i of the caller's table goes to context i mod n_ctx (interleaved: per-point cost correlates with s and theta,
// so contiguous blocks of a sorted table would load one GPU with all the expensive points).  One host thread per
// context gathers its shard, runs the ordinary single-device call and scatters its rows back into the caller's
// [n][8] table; there is no exchange between devices while they compute, and a point's result does not depend on
// which device evaluated it, so the table is bit-identical for every n_ctx.  Contexts that sit on the SAME device
// (a 1-GPU box rehearsing the path) run one after the other: two persistent grids on one device time-slice badly.
static std::mutex g_device_mu[64];

extern "C" int rimphony_batch_compute_multi(rimphony_ctx *const *ctxs, int n_ctx, int kind, size_t n,
                                            const double *s, const double *theta, const double *const *params,
                                            uint32_t coeff_mask, int precision, double *out, int32_t *status, uint64_t *work)
{
    if (!ctxs || n_ctx < 1 || n_ctx > 64) return RIMPHONY_EINVAL;
    for (int r = 0; r < n_ctx; r++) if (!ctxs[r]) return RIMPHONY_EINVAL;
    bool empty;
    const int rc0 = check_batch_args(kind, { params }, ctxs[0], precision, n, &empty, { s, theta, out }, params);
    if (rc0 || empty) return rc0;
    const int np = NPARAMS[kind];
    if (n_ctx == 1) return rimphony_batch_compute_ex(ctxs[0], kind, n, s, theta, params, coeff_mask, precision, out, status, work);

    std::vector<int> rcs((size_t) n_ctx, RIMPHONY_OK);
    std::vector<std::string> errs((size_t) n_ctx);
    auto run = [&](int r) {
        const size_t m = (n - (size_t) r + (size_t) n_ctx - 1) / (size_t) n_ctx;      // rows r, r + n_ctx, ...
        if (m == 0) return;
        try {
            std::vector<double> in((size_t) (2 + np) * m), o(m * 8);
            std::vector<int32_t> stt(status ? m * 8 : 0);
            std::vector<uint64_t> wk(work ? m * 8 : 0);
            const double *pp[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
            for (size_t j = 0; j < m; j++) {
                const size_t i = (size_t) r + j * (size_t) n_ctx;
                in[j] = s[i];
                in[m + j] = theta[i];
                for (int k = 0; k < np; k++) in[(size_t) (2 + k) * m + j] = params[k][i];
            }
            for (int k = 0; k < np; k++) pp[k] = in.data() + (size_t) (2 + k) * m;
            int rc;
            {
                const int dev = ctxs[r]->device;
                std::lock_guard<std::mutex> same_device(g_device_mu[dev & 63]);
                rc = rimphony_batch_compute_ex(ctxs[r], kind, m, in.data(), in.data() + m, pp, coeff_mask, precision,
                                               o.data(), status ? stt.data() : nullptr, work ? wk.data() : nullptr);
            }
            if (rc) { rcs[(size_t) r] = rc; errs[(size_t) r] = rimphony_last_error(); return; }
            for (size_t j = 0; j < m; j++) {
                const size_t i = (size_t) r + j * (size_t) n_ctx;
                memcpy(out + i * 8, o.data() + j * 8, 8 * sizeof(double));
                if (status) memcpy(status + i * 8, stt.data() + j * 8, 8 * sizeof(int32_t));
                if (work) memcpy(work + i * 8, wk.data() + j * 8, 8 * sizeof(uint64_t));
            }
        } catch (const std::bad_alloc &) {
            rcs[(size_t) r] = RIMPHONY_ENOMEM;
        }
    };
    std::vector<std::thread> threads;
    try {
        for (int r = 1; r < n_ctx; r++) threads.emplace_back(run, r);
    } catch (...) {
        for (auto &t : threads) t.join();
        return RIMPHONY_ENOMEM;
    }
    run(0);
    for (auto &t : threads) t.join();
    for (int r = 0; r < n_ctx; r++)
        if (rcs[(size_t) r]) {
            if (!errs[(size_t) r].empty()) rim_set_last_error("rimphony_batch_compute_multi", errs[(size_t) r].c_str());
            return rcs[(size_t) r];
        }
    return RIMPHONY_OK;
}

// Where did the coefficients of a table end?  hist[slot][b] = number of rows whose status word of that slot has bit b
// set (b = 0..6: the RIMPHONY_ST_* bits), hist[slot][7] = rows with status 0.
__global__ void status_hist_kernel(const int32_t *status, size_t n, unsigned long long *hist)
{
    __shared__ unsigned h[64];
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < n * 8; idx += (size_t) gridDim.x * blockDim.x) {
        const int slot = (int) (idx & 7);
        const int v = status[idx];
        if (v == 0) atomicAdd(&h[slot * 8 + 7], 1u);
        for (int b = 0; b < 7; b++) if (v & (1 << b)) atomicAdd(&h[slot * 8 + b], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64 && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long) h[threadIdx.x]);
}

extern "C" int rimphony_status_histogram_device(rimphony_ctx *c, size_t n, const int32_t *d_status, uint64_t hist[64], void *stream)
{
    if (!c || !hist) return RIMPHONY_EINVAL;
    for (int k = 0; k < 64; k++) hist[k] = 0;
    if (n == 0) return RIMPHONY_OK;
    if (!d_status) return RIMPHONY_EINVAL;
    std::lock_guard<std::recursive_mutex> lock(*c->mu);
    rim_clear_last_error();
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t) stream;
    // the histogram words live behind the counter words of the queue allocation? no: they are read back here, so a
    // private scratch allocation keeps this call independent of a batch in flight
    unsigned long long *d_hist = nullptr;
    if (hipMalloc(&d_hist, 64 * sizeof(unsigned long long)) != hipSuccess) return RIMPHONY_ENOMEM;
    int rc = RIMPHONY_OK;
    if (hipMemsetAsync(d_hist, 0, 64 * sizeof(unsigned long long), st) != hipSuccess) rc = RIMPHONY_EHIP;
    if (!rc) {
        const size_t total = n * 8;
        const unsigned blocks = (unsigned) ((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
        hipLaunchKernelGGL(status_hist_kernel, dim3(blocks), dim3(256), 0, st, d_status, n, d_hist);
        if (hipGetLastError() != hipSuccess) rc = RIMPHONY_EHIP;
    }
    if (!rc && hipMemcpyAsync(hist, d_hist, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) rc = RIMPHONY_EHIP;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = RIMPHONY_EHIP;
    (void) hipFree(d_hist);
    if (rc == RIMPHONY_EHIP) rim_set_last_error("rimphony_status_histogram_device", "HIP call failed");
    return rc;
}

extern "C" int rimphony_highfreq_batch_device(rimphony_ctx *c, int kind, size_t n, const double *d_s, const double *d_theta,
                                              const double *const *d_params, double *d_out, void *stream);

// host-buffer form of rimphony_highfreq_batch_device (out: [n][2] = rho_Q, rho_V)
extern "C" int rimphony_highfreq_batch(rimphony_ctx *c, int kind, size_t n, const double *s, const double *theta,
                                       const double *const *params, double *out)
{
    if (!c || !params) return RIMPHONY_EINVAL;
    if (kind != RIMPHONY_POWER_LAW && kind != RIMPHONY_THERMAL_JUETTNER) return RIMPHONY_EINVAL;
    if (n == 0) return RIMPHONY_OK;
    if (!s || !theta || !out) return RIMPHONY_EINVAL;
    RimCtxScope scope(c, nullptr);
    {
        const int rc0 = scope.enter();
        if (rc0) return rc0;
        if (c->ev_batch_valid) HIP_TRY(hipEventSynchronize(c->ev_batch));   // the staging buffer may still be in use
    }
    const int np = kind == RIMPHONY_POWER_LAW ? 2 : 1;       // only p and gamma_min (or T) enter the closed forms
    for (int k = 0; k < np; k++) if (!params[k]) return RIMPHONY_EINVAL;
    const size_t need_in = n * (size_t) (2 + np + 2);
    { const int rcb = c->d_in.grow(need_in, need_in * sizeof(double), "the staged inputs"); if (rcb) return rcb; }
    HIP_TRY(hipMemcpy(c->d_in.p, s, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_in.p + n, theta, n * sizeof(double), hipMemcpyHostToDevice));
    const double *dp[2] = { nullptr, nullptr };
    for (int k = 0; k < np; k++) {
        HIP_TRY(hipMemcpy(c->d_in.p + (size_t) (2 + k) * n, params[k], n * sizeof(double), hipMemcpyHostToDevice));
        dp[k] = c->d_in.p + (size_t) (2 + k) * n;
    }
    double *d_res = c->d_in.p + (size_t) (2 + np) * n;
    const int rc = rimphony_highfreq_batch_device(c, kind, n, c->d_in.p, c->d_in.p + n, dp, d_res, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_res, n * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return RIMPHONY_OK;
}

extern "C" int rimphony_bessel_batch_device(rimphony_ctx *c, size_t count, const double *d_n, const double *d_x,
                                            double *d_j, double *d_dj, void *stream)
{
    if (!c || (count && (!d_n || !d_x))) return RIMPHONY_EINVAL;
    if (count == 0) return RIMPHONY_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(bessel_kernel, dim3((unsigned) ((count + 255) / 256)), dim3(256), 0, (hipStream_t) stream,
                       count, d_n, d_x, d_j, d_dj);
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

// ---- the reference's scalar FFI seam (leung-bessel/src/lib.rs:36-42, 56-75) -------------------
// `extern { fn pkgw_bessel_j(n: c_double, x: c_double) -> c_double; fn pkgw_bessel_dj(..) }`: the same two C symbols,
// so the reference's leung-bessel crate can link this library instead of bessel.c.  They are the HOST build of the
// very functions the kernels inline (dev_bessel.h is __host__ __device__): no HIP call, no GPU needed, reentrant,
// a few hundred nanoseconds per call like the C code they replace, and -- the rounding contract of detmath.h --
// the same bits as rimphony_bessel_batch_device returns for the same arguments.  Errors are NaN, as in bessel.c.
extern "C" double pkgw_bessel_j(double n, double x) { return rim::bessel_j(n, x); }
extern "C" double pkgw_bessel_dj(double n, double x) { return rim::bessel_dj(n, x); }

static int fill_point_args(const rimphony_ctx *c, int kind, const double *params, int coeff, int stokes, int negative_lobe,
                           double s, double theta, PointArgs &pa)
{
    if (kind < 0 || kind > RIMPHONY_TABULATED || !params) return RIMPHONY_EINVAL;
    if (coeff < 0 || coeff > 1 || stokes < 0 || stokes > 2) return RIMPHONY_EINVAL;
    if (check_tables(c, kind)) return RIMPHONY_EINVAL;
    for (int k = 0; k < 5; k++) pa.par[k] = (k < NPARAMS[kind]) ? params[k] : 0.;
    if (kind == RIMPHONY_TABULATED) pa.par[1] = rim_frombits((uint64_t) (uintptr_t) c->d_tab.p);     // (as load_params)
    pa.s = s; pa.theta = theta; pa.coeff = coeff; pa.stokes = stokes; pa.negative_lobe = negative_lobe;
    return RIMPHONY_OK;
}

// normalisation of a single host-described point -> c->d_norm.p[0]
static int single_point_norm(rimphony_ctx *c, int kind, const double *params, hipStream_t st)
{
    int rc = ensure_norm(c, 8);
    if (rc) return rc;
    // params live in d_norm[1..5] as five 1-element SoA arrays
    double h[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int k = 0; k < NPARAMS[kind]; k++) h[1 + k] = params[k];
    HIP_TRY(hipMemcpyAsync(c->d_norm.p, h, sizeof h, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // h is a stack buffer
    ParamPtrs pp;
    for (int k = 0; k < 5; k++) pp.p[k] = c->d_norm.p + 1 + k;
    if (kind == RIMPHONY_TABULATED) pp.p[1] = c->d_tab.p;
    rc = family_lines(c, kind, 1, pp);
    if (rc) return rc;
    return launch_norm(c, kind, 1, pp, c->d_norm.p, st);
}

// the one entry path of the per-point seams (rimphony_internal.h)
int RimPointSeam::begin(rimphony_ctx *c, int kind_, const double *params, int coeff, int stokes, int negative_lobe, double s,
                        double theta, size_t count, int waves_per_cu, void *stream)
{
    int rc = fill_point_args(c, kind_, params, coeff, stokes, negative_lobe, s, theta, pa);
    if (rc || count == 0) return rc;
    st = (hipStream_t) stream;
    scope.emplace(c, st);              // the context's lock; enter() selects c->device and orders st behind earlier work
    rc = scope->enter();
    if (rc) return rc;
    rc = single_point_norm(c, kind_, params, st);
    if (rc) return rc;
    // (a family with a sin^k prefactor or of 2-D surfaces: the point's line, which the normalisation has just written --
    // dist_of reads par[2])
    if (kind_ == RIMPHONY_TABULATED && tab_kind_has_lines(c->tab_kind))
        pa.par[2] = rim_frombits((uint64_t) (uintptr_t) c->d_famline.p);
    if (waves_per_cu) {
        grid = persistent_grid(c, count, waves_per_cu);
        rc = ensure_spill(c, grid);
        if (rc) return rc;
    } else grid = (unsigned) ((count + 63) / 64);
    norm = c->d_norm.p;
    spill = c->d_spill.p;
    kind = kind_ == RIMPHONY_TABULATED ? rim_tab_seam_kind(c->tab_kind) : kind_;
    return RIMPHONY_OK;
}

extern "C" int rimphony_gamma_integrand_batch_device(rimphony_ctx *c, int kind, const double *params,
                                                     int coeff, int stokes, double s, double theta,
                                                     size_t count, const double *d_n, const double *d_gamma,
                                                     double *d_out, void *stream)
{
    if (!c || (count && (!d_n || !d_gamma || !d_out))) return RIMPHONY_EINVAL;
    RimPointSeam m;
    const int rc = m.begin(c, kind, params, coeff, stokes, 0, s, theta, count, 0, stream);
    if (rc || !count) return rc;
    if (kind == RIMPHONY_TABULATED) rim_tab_launch_integrand(m.kind, m.grid, m.st, m.pa, m.norm, count, d_n, d_gamma, d_out);
    else rim_with_kind(kind, [&](auto K) { hipLaunchKernelGGL(integrand_kernel_n<decltype(K)::value>, dim3(m.grid), dim3(64), RIM_DYN_LDS, m.st, m.pa, m.norm, count, d_n, d_gamma, d_out); });
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

extern "C" int rimphony_gamma_integral_batch_device(rimphony_ctx *c, int kind, const double *params,
                                                    int coeff, int stokes, int negative_lobe, double s, double theta,
                                                    size_t count, const double *d_n, double *d_out, void *stream)
{
    if (!c || (count && (!d_n || !d_out))) return RIMPHONY_EINVAL;
    RimPointSeam m;
    const int rc = m.begin(c, kind, params, coeff, stokes, negative_lobe, s, theta, count, 16, stream);
    if (rc || !count) return rc;
    if (kind == RIMPHONY_TABULATED) rim_tab_launch_gamma_integral(m.kind, m.grid, m.st, m.pa, m.norm, count, d_n, d_out, m.spill);
    else rim_with_kind(kind, [&](auto K) { hipLaunchKernelGGL(gamma_integral_kernel<decltype(K)::value>, dim3(m.grid), dim3(64), RIM_DYN_LDS, m.st, m.pa, m.norm, count, d_n, d_out, m.spill); });
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

// ---- unit seam for the leaf functions of detmath.h ------------------------------------------
__global__ void detmath_kernel(int op, size_t n, const double *x, const double *y, double *out)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = x[i], b = y ? y[i] : 0.;
    double r, t;
    switch (op) {
    case 0: r = rim_exp(a); break;
    case 1: r = rim_log(a); break;
    case 2: r = rim_log10(a); break;
    case 3: r = rim_pow(a, b); break;
    case 4: r = rim_sqrt(a); break;
    case 5: r = rim_log10_region(a); break;
    case 6: r = rim_lgamma_pos(a); break;
    case 7: rim_sincos(a, &r, &t); break;
    case 8: rim_sincos(a, &t, &r); break;
    case 9: r = rim_div_by(a, b, 1. / b); break;
    case 10: r = rim_cbrt_normal(a); break;
    case 11: r = rim_rgamma_near(a); break;
    case 12: { double o4[4]; rim_third_powers(a, o4); const int j = (int) b; r = j == 0 ? o4[0] : j == 1 ? o4[1] : j == 2 ? o4[2] : o4[3]; break; }
    case 13: r = rim_rqrt4_normal(a); break;
    case 14: r = rim_powexp_normal(a, b, -a * 1e-3); break;
    default: r = RIM_NAN; break;
    }
    out[i] = r;
}

extern "C" int rimphony_detmath_batch_device(rimphony_ctx *c, int op, size_t n, const double *d_x, const double *d_y,
                                             double *d_out, void *stream)
{
    if (!c || op < 0 || op > 14) return RIMPHONY_EINVAL;
    if (n == 0) return RIMPHONY_OK;
    if (!d_x || !d_out || ((op == 3 || op == 9 || op == 12 || op == 14) && !d_y)) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(detmath_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, op, n, d_x, d_y, d_out);
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

// ---- high-frequency closed forms ---------------------------------------------
__global__ void highfreq_kernel(int kind, size_t n, const double *s, const double *theta, const double *p0,
                                const double *p1, double *out)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sn, cs;
    rim_sincos(theta[i], &sn, &cs);
    double q, v;
    if (kind == RIMPHONY_POWER_LAW) {
        q = rim_hf_powerlaw_faraday_q(p0[i], p1[i], s[i], sn);
        v = rim_hf_powerlaw_faraday_v(p0[i], p1[i], s[i], sn);
    } else {
        rim_hf_thermal_faraday(p0[i], s[i], sn, cs, &q, &v);
    }
    out[2 * i] = q;
    out[2 * i + 1] = v;
}

extern "C" int rimphony_highfreq_batch_device(rimphony_ctx *c, int kind, size_t n, const double *d_s, const double *d_theta,
                                              const double *const *d_params, double *d_out, void *stream)
{
    if (!c) return RIMPHONY_EINVAL;
    if (kind != RIMPHONY_POWER_LAW && kind != RIMPHONY_THERMAL_JUETTNER) return RIMPHONY_EINVAL;
    if (n == 0) return RIMPHONY_OK;
    if (!d_s || !d_theta || !d_params || !d_out || !d_params[0]) return RIMPHONY_EINVAL;
    if (kind == RIMPHONY_POWER_LAW && !d_params[1]) return RIMPHONY_EINVAL;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(highfreq_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, kind, n,
                       d_s, d_theta, d_params[0], kind == RIMPHONY_POWER_LAW ? d_params[1] : nullptr, d_out);
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}

extern "C" int rimphony_qag_selftest_device(rimphony_ctx *c, size_t count, const int32_t *d_family,
                                            const double *d_p0, const double *d_p1, const double *d_a, const double *d_b,
                                            double epsabs, double epsrel, int32_t limit,
                                            double *d_result, double *d_abserr, int32_t *d_qstatus, int32_t *d_size,
                                            void *stream)
{
    if (!c || (count && (!d_family || !d_p0 || !d_p1 || !d_a || !d_b || !d_result || !d_abserr || !d_qstatus || !d_size)))
        return RIMPHONY_EINVAL;
    if (limit < 1) return RIMPHONY_EINVAL;
    if (count == 0) return RIMPHONY_OK;
    RimCtxScope scope(c, (hipStream_t) stream);
    int rc = scope.enter();
    if (rc) return rc;
    const unsigned grid = persistent_grid(c, count, 16);
    rc = ensure_spill(c, grid);
    if (rc) return rc;
    hipLaunchKernelGGL(qag_selftest_kernel, dim3(grid), dim3(64), 0, (hipStream_t) stream, count, d_family, d_p0, d_p1,
                       d_a, d_b, epsabs, epsrel, (int) limit, d_result, d_abserr, d_qstatus, d_size, c->d_spill.p);
    HIP_TRY(hipGetLastError());
    return RIMPHONY_OK;
}
