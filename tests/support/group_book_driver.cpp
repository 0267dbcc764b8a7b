// CPU emulation driver: the booking of one turn of the group quadrature (symphony_group.h) on 64 host threads --
// group_book member by member against group_book_turn (group_book_lanes and its fallback) on identical LDS images
// (tests only).
#define RIM_WAVE_EMU 1
#include <cstdio>
#include <cstring>
#include "../../rimphony_amd/csrc/symphony_wave.h"
namespace rim { unsigned long long g_emu_hist[64]; }
#include "../../rimphony_amd/csrc/symphony_group.h"

using namespace rim;

#define LIST_DOUBLES (RIM_GROUP * RIM_ISTORE_DOUBLES(CAP_GINNER))
#define SPILL_DOUBLES (RIM_GROUP * RIM_ISTORE_DOUBLES(SPILL_GINNER))

struct BookImage {
    GroupParkBase gp;
    double lists[LIST_DOUBLES];
    double spill[SPILL_DOUBLES];
    unsigned finished, need_pick;
    int lanes;                  // mode 2: did group_book_lanes take the turn?
};

struct BookTask {
    BookImage *img;
    int mode;                   // 0: group_book member by member, 1: group_book_turn, 2: group_book_lanes alone
    int cur, stash, limit;
    unsigned set, posp;
    double epsrel;
};

static void book_lane_body(BookTask *t)
{
    __shared__ double s_tab[96];
    const GKLane g = gk_lane_init(s_tab);
    BookImage *const im = t->img;
    GroupBooked bk;
    bk.finished = 0; bk.need_pick = 0;
    int lanes = 0;
    if (t->mode == 0) {
        for (unsigned rem = t->set; rem; rem &= rem - 1) {
            const int m = __builtin_ctz(rem);
            const IStore st = group_store(im->lists, CAP_GINNER, im->spill, SPILL_GINNER, m);
            if (group_book_filed(&im->gp, st, g, t->cur, m, t->stash != 0, (int) ((t->posp >> (4 * m)) & (RIM_STASH - 1)),
                                 t->epsrel, t->limit)) bk.finished |= 1u << m;
            else bk.need_pick |= 1u << m;
        }
    } else if (t->mode == 1) {
        bk = group_book_turn(&im->gp, im->lists, im->spill, g, t->cur, t->set, t->stash != 0, t->posp, t->epsrel, t->limit);
    } else {
        lanes = group_book_lanes(&im->gp, im->lists, g, t->cur, t->set, t->stash != 0, t->posp, t->epsrel, t->limit, bk) ? 1 : 0;
    }
    wv_sync();
    if (g.lane == 0) { im->finished = bk.finished; im->need_pick = bk.need_pick; im->lanes = lanes; }
}

struct BookThreadArg { BookTask *t; int lane; };

static void *book_thread_main(void *p)
{
    BookThreadArg *a = (BookThreadArg *) p;
    emu_lane_ref() = a->lane;
    book_lane_body(a->t);
    return nullptr;
}

static void run_wave(BookTask *t)
{
    pthread_barrier_init(&emu_wave().bar, nullptr, 64);
    pthread_t th[64];
    BookThreadArg args[64];
    for (int i = 0; i < 64; i++) {
        args[i].t = t; args[i].lane = i;
        pthread_create(&th[i], nullptr, book_thread_main, &args[i]);
    }
    for (int i = 0; i < 64; i++) pthread_join(th[i], nullptr);
    pthread_barrier_destroy(&emu_wave().bar);
}

extern "C" int emu_group_member_size() { return (int) sizeof(GroupMember); }
extern "C" int emu_group_list_doubles() { return RIM_ISTORE_DOUBLES(CAP_GINNER); }
extern "C" int emu_group_spill_doubles() { return RIM_ISTORE_DOUBLES(SPILL_GINNER); }

// members: RIM_GROUP GroupMember records; lists: the members' LDS lists; spill: their spill regions (all three are
// inputs and, from the group_book_turn run, outputs).  out[0..1]: finished / need-pick masks of group_book, out[2..3]: of
// group_book_turn, out[4]: 1 if group_book_lanes took the turn.  Returns a mask of what differs between the two images:
// 1 member records, 2 lists, 4 spill regions.
extern "C" int emu_group_book_compare(void *members, double *lists, double *spill, int cur, unsigned set, int stash, unsigned posp,
                                      double epsrel, int limit, unsigned *out)
{
    static BookImage ref, lan, probe;
    BookImage *const imgs[3] = { &ref, &lan, &probe };
    for (int k = 0; k < 3; k++) {
        std::memset(&imgs[k]->gp, 0, sizeof(GroupParkBase));
        std::memcpy(imgs[k]->gp.mem, members, sizeof(GroupMember) * RIM_GROUP);
        std::memcpy(imgs[k]->lists, lists, sizeof(double) * LIST_DOUBLES);
        std::memcpy(imgs[k]->spill, spill, sizeof(double) * SPILL_DOUBLES);
        BookTask t;
        t.img = imgs[k]; t.mode = k; t.cur = cur; t.stash = stash; t.limit = limit; t.set = set; t.posp = posp; t.epsrel = epsrel;
        run_wave(&t);
    }
    int diff = 0;
    if (std::memcmp(ref.gp.mem, lan.gp.mem, sizeof(GroupMember) * RIM_GROUP)) diff |= 1;
    if (std::memcmp(ref.lists, lan.lists, sizeof(double) * LIST_DOUBLES)) diff |= 2;
    if (std::memcmp(ref.spill, lan.spill, sizeof(double) * SPILL_DOUBLES)) diff |= 4;
    out[0] = ref.finished; out[1] = ref.need_pick; out[2] = lan.finished; out[3] = lan.need_pick; out[4] = (unsigned) probe.lanes;
    std::memcpy(members, lan.gp.mem, sizeof(GroupMember) * RIM_GROUP);
    std::memcpy(lists, lan.lists, sizeof(double) * LIST_DOUBLES);
    std::memcpy(spill, lan.spill, sizeof(double) * SPILL_DOUBLES);
    return diff;
}
