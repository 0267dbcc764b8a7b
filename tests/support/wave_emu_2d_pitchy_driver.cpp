// CPU emulation driver for the tabulated distribution as a 2-D set with a sin^k xi prefactor: a whole Symphony group
// (symphony_group.h) of DIST_TABULATED_2D_PITCHY or DIST_TABULATED_2D_GRID_PITCHY on the 64-thread wavefront emulator, the
// counterpart of wave_emu_2d_grid_driver.cpp for the two forms whose samples evaluate a bicubic and the factor's pow
// (dev_symphony.h: tab_calc_f_both).  It reuses the analytic driver's lane body, which is templated on the kind
// (tests/debugging only).
#include "wave_emu_driver.cpp"

template <int KIND>
static void *pitchy2d_group_thread_main(void *p)
{
    ThreadArg *a = (ThreadArg *) p;
    EmuGroupTask *t = (EmuGroupTask *) (void *) a->t;
    emu_lane_ref() = a->lane;
    group_lane_body<KIND>(t);
    return nullptr;
}

// form: 10 (nodes uniform in ln gamma) or 11 (given nodes); par[0] the table index, par[1] the bits of the set's host address;
// the rest as emu_symphony_group.  Returns 1 if every lane ended with the same values.
extern "C" int emu_symphony_group_2d_pitchy(int form, unsigned slots, int nmem, double s, double theta, const double *par, double norm,
                                            double *vals, int *stats, unsigned long long *work4)
{
    static EmuGroupTask t;
    const bool on_grid = form == DIST_TABULATED_2D_GRID_PITCHY;
    t.kind = on_grid ? DIST_TABULATED_2D_GRID_PITCHY : DIST_TABULATED_2D_PITCHY;
    t.nmem = nmem; t.slots = slots; t.s = s; t.theta = theta; t.norm = norm;
    for (int k = 0; k < 5; k++) t.par[k] = par[k];
    pthread_barrier_init(&emu_wave().bar, nullptr, 64);
    pthread_t th[64];
    ThreadArg args[64];
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, 1 << 20);
    for (int i = 0; i < 64; i++) {
        args[i].t = (EmuTask *) (void *) &t; args[i].lane = i;
        pthread_create(&th[i], &attr, on_grid ? pitchy2d_group_thread_main<DIST_TABULATED_2D_GRID_PITCHY>
                                              : pitchy2d_group_thread_main<DIST_TABULATED_2D_PITCHY>, &args[i]);
    }
    for (int i = 0; i < 64; i++) pthread_join(th[i], nullptr);
    pthread_barrier_destroy(&emu_wave().bar);
    int uniform = 1;
    for (int i = 1; i < 64; i++)
        for (int m = 0; m < nmem; m++)
            if (std::memcmp(&t.vals[i][m], &t.vals[0][m], 8) != 0 || t.stats[i][m] != t.stats[0][m]) uniform = 0;
    for (int m = 0; m < nmem; m++) { vals[m] = t.vals[0][m]; stats[m] = t.stats[0][m]; }
    work4[0] = t.samples; work4[1] = t.passes; work4[2] = t.inner_qags; work4[3] = t.member_passes; work4[4] = t.stash_filed;
    for (int k = 0; k < 40; k++) rim::g_emu_hist[k] = 0;
    return uniform;
}
