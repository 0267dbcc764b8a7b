// CPU emulation driver: the members' part of one pass of the group quadrature (symphony_group.h) on 64 host threads --
// the rule applied member by member with lanes 0 / 32 filing (wave_gk31 per served member: the form this kernel had
// before the members' rule-sum tails ran side by side, restated here as the reference) against group_rule_sums on
// identical LDS images and identical per-lane sample vectors (tests only).
#define RIM_WAVE_EMU 1
#include <cstdio>
#include <cstring>
#include "../../rimphony_amd/csrc/symphony_wave.h"
namespace rim { unsigned long long g_emu_hist[64]; }
#include "../../rimphony_amd/csrc/symphony_group.h"

using namespace rim;

// the integrand's member step: member m's sample of this lane from a table [RIM_GROUP][64]
struct TableF {
    const double *fv;
    int lane;
    double member(int m, bool active) const { return active ? fv[64 * m + lane] : 0.; }
};

struct TailCounts { unsigned stashed, n_samp_all, n_member_pass, n_qags, n_filed; };

struct TailImage {
    GroupParkBase gp;
    TailCounts cnt;
};

struct TailTask {
    TailImage *img;
    const double *fv;
    int mode;                   // 0: member by member, 1: group_rule_sums
    int cur;
    unsigned serve, booknow, maskA, maskB;
    unsigned long long idxp;
    double hl[2];               // half-length of the interval of half-wave 0 / 1
    TailCounts cnt0;            // the counters before the pass
};

// The member loop of a pass as it was: every served member's rule applied whole, lanes 0 and 32 filing.
template <class F>
static void member_by_member(F &f, const GKLane &g, GroupParkBase *gp, int cur, unsigned serve, unsigned booknow,
                             unsigned long long idxp, unsigned maskA, unsigned maskB, double hl, TailCounts &c)
{
    const int lane = g.lane;
    for (unsigned rem = serve; rem; rem &= rem - 1) {
        const int m = __builtin_ctz(rem);
        GroupMember *const M = gp->mem + m;
        const bool inA = ((maskA >> m) & 1u) != 0, inB = ((maskB >> m) & 1u) != 0;
        const bool act_m = cur < 0 ? (g.node && (g.half == 0 ? inA : inB)) : g.node;
        const double fv = f.member(m, act_m);
        const GKRes r = wave_gk31(fv, hl, g);
        if (cur < 0) {
            if ((lane == 0 && inA) || (lane == 32 && inB)) {
                double *fb = M->fb[g.half];
                fb[0] = r.result; fb[1] = r.abserr; fb[2] = r.resabs; fb[3] = r.resasc;
            }
            const unsigned ns = (inA ? 31u : 0u) + (inB ? 31u : 0u);
            if (lane == 0) M->samples = ns;
            c.n_samp_all += ns;
            c.n_member_pass += 1;
            c.n_qags += (inA ? 1u : 0u) + (inB ? 1u : 0u);
        } else {
            const unsigned long long ne = wv_ballot(r.resasc != r.abserr);
            if ((booknow >> m) & 1u) {
                if (g.j == 0) {
                    double *h = M->fb[cur] + 2 * g.half;
                    h[0] = r.result; h[1] = r.abserr;
                    if (!g.half) M->hf = (int) (ne & 1ull) | (int) (((ne >> 32) & 1ull) << 1);
                }
            } else {
                const int idx = (int) ((idxp >> (16 * m)) & 0xffffull);
                const unsigned long long freep = wv_ballot(lane < RIM_STASH && M->sk[lane & (RIM_STASH - 1)] < 0);
                const int pos = freep ? __builtin_ffsll((long long) freep) - 1 : uni(M->snext);
                wv_sync();
                if (lane == 0) {
                    M->sk[pos] = idx;
                    M->sf[pos] = (int) (ne & 1ull) | (int) (((ne >> 32) & 1ull) << 1);
                    M->sr1[pos] = r.result; M->se1[pos] = r.abserr;
                    if (!freep) M->snext = (pos + 1) & (RIM_STASH - 1);
                }
                if (lane == 32) { M->sr2[pos] = r.result; M->se2[pos] = r.abserr; }
                c.stashed |= 1u << m;
                c.n_filed += 1;
            }
        }
    }
}

static void tail_lane_body(TailTask *t)
{
    __shared__ double s_tab[96];
    const GKLane g = gk_lane_init(s_tab);
    TailImage *const im = t->img;
    TableF f;
    f.fv = t->fv; f.lane = g.lane;
    TailCounts c = t->cnt0;
    const double hl = t->hl[g.half];
    if (t->mode == 0) member_by_member(f, g, &im->gp, t->cur, t->serve, t->booknow, t->idxp, t->maskA, t->maskB, hl, c);
    else group_rule_sums(f, g, &im->gp, t->cur, t->serve, t->booknow, t->idxp, t->maskA, t->maskB, hl,
                         c.stashed, c.n_samp_all, c.n_member_pass, c.n_qags, c.n_filed);
    wv_sync();
    if (g.lane == 0) im->cnt = c;
}

struct TailThreadArg { TailTask *t; int lane; };

static void *tail_thread_main(void *p)
{
    TailThreadArg *a = (TailThreadArg *) p;
    emu_lane_ref() = a->lane;
    tail_lane_body(a->t);
    return nullptr;
}

static void run_wave(TailTask *t)
{
    pthread_barrier_init(&emu_wave().bar, nullptr, 64);
    pthread_t th[64];
    TailThreadArg args[64];
    for (int i = 0; i < 64; i++) {
        args[i].t = t; args[i].lane = i;
        pthread_create(&th[i], nullptr, tail_thread_main, &args[i]);
    }
    for (int i = 0; i < 64; i++) pthread_join(th[i], nullptr);
    pthread_barrier_destroy(&emu_wave().bar);
}

extern "C" int emu_group_member_size() { return (int) sizeof(GroupMember); }

// members: RIM_GROUP GroupMember records (input; output: the records after group_rule_sums); fv: the members' samples
// [RIM_GROUP][64]; hl[2]: the half-lengths of the two half-waves' intervals; counts[5]: stashed, n_samp_all,
// n_member_pass, n_qags, n_filed before the pass (input) and after group_rule_sums (output).  Returns a mask of what
// differs between the two forms: 1 member records, 2 counters.
extern "C" int emu_group_rule_tails_compare(void *members, const double *fv, int cur, unsigned serve, unsigned booknow,
                                            unsigned long long idxp, unsigned maskA, unsigned maskB, const double *hl,
                                            unsigned *counts)
{
    static TailImage ref, lan;
    TailImage *const imgs[2] = { &ref, &lan };
    for (int k = 0; k < 2; k++) {
        std::memset(imgs[k], 0, sizeof(TailImage));
        std::memcpy(imgs[k]->gp.mem, members, sizeof(GroupMember) * RIM_GROUP);
        TailTask t;
        t.img = imgs[k]; t.fv = fv; t.mode = k; t.cur = cur; t.serve = serve; t.booknow = booknow;
        t.maskA = maskA; t.maskB = maskB; t.idxp = idxp; t.hl[0] = hl[0]; t.hl[1] = hl[1];
        t.cnt0.stashed = counts[0]; t.cnt0.n_samp_all = counts[1]; t.cnt0.n_member_pass = counts[2];
        t.cnt0.n_qags = counts[3]; t.cnt0.n_filed = counts[4];
        run_wave(&t);
    }
    int diff = 0;
    if (std::memcmp(ref.gp.mem, lan.gp.mem, sizeof(GroupMember) * RIM_GROUP)) diff |= 1;
    if (std::memcmp(&ref.cnt, &lan.cnt, sizeof(TailCounts))) diff |= 2;
    std::memcpy(members, lan.gp.mem, sizeof(GroupMember) * RIM_GROUP);
    counts[0] = lan.cnt.stashed; counts[1] = lan.cnt.n_samp_all; counts[2] = lan.cnt.n_member_pass;
    counts[3] = lan.cnt.n_qags; counts[4] = lan.cnt.n_filed;
    return diff;
}

// One application of the rule (wave_gk31) to given node values, for the test to see which branches of rescale_error its
// sample vectors take: out[8] = result, abserr, resabs, resasc of half-wave 0 and of half-wave 1.
struct RuleTask { const double *fv; double hl[2]; double out[8]; };

static void *rule_thread_main(void *p)
{
    TailThreadArg *a = (TailThreadArg *) p;
    emu_lane_ref() = a->lane;
    RuleTask *t = (RuleTask *) (void *) a->t;
    __shared__ double s_tab[96];
    const GKLane g = gk_lane_init(s_tab);
    const GKRes w = wave_gk31(g.node ? t->fv[g.lane] : 0., t->hl[g.half], g);
    if (g.j == 0) { double *o = t->out + 4 * g.half; o[0] = w.result; o[1] = w.abserr; o[2] = w.resabs; o[3] = w.resasc; }
    return nullptr;
}

extern "C" void emu_rule_apply(const double *fv, const double *hl, double *out)
{
    static RuleTask t;
    t.fv = fv; t.hl[0] = hl[0]; t.hl[1] = hl[1];
    pthread_barrier_init(&emu_wave().bar, nullptr, 64);
    pthread_t th[64];
    TailThreadArg args[64];
    for (int i = 0; i < 64; i++) {
        args[i].t = (TailTask *) (void *) &t; args[i].lane = i;
        pthread_create(&th[i], nullptr, rule_thread_main, &args[i]);
    }
    for (int i = 0; i < 64; i++) pthread_join(th[i], nullptr);
    pthread_barrier_destroy(&emu_wave().bar);
    std::memcpy(out, t.out, sizeof(t.out));
}
