"""GPU test of the tabulated distribution's one installer (rimphony_hip.hip: install_tables): the five forms of a table set
installed one after the other in every order of two, on the default routing and one wave per coefficient, and cleared
through each of the five entries.  A form's DIST_TABULATED* value is the installer's record of it, the cell of the
context's occupancy caches and the argument of every kernel lookup, so each ordered pair of forms is a case of its own.
The launches run under a time limit of their own."""
import ctypes
import functools
import os

import numpy as np
import pytest

import tab_grid_bind as tg
from test_gpu_tabulated_group import GOLDEN, TAB, env_context, form_case, same_bits, time_limit

pytestmark = pytest.mark.gpu

FORMS = ("isotropic", "pitch", "2-D", "sin^k", "given nodes")
ROWS, MASK = 4, 0x3F
# an Euler circuit of the complete directed graph on the five forms: a first install, then 20, in which each form follows
# each other form directly once (the four cycles i -> i + d mod 5, d = 1 .. 4, from form 0)
SEQUENCE = [0] + [(d * i) % 5 for d in (1, 2, 3, 4) for i in (1, 2, 3, 4, 5)]


@functools.lru_cache(maxsize=None)
def cases():
    """form -> (install(ctx), s, theta, index, values [ROWS][6]): the committed fixtures' sets and first rows"""
    res = {}
    for form in FORMS[:4]:
        install, s, th, index, values, _ = form_case(form)
        res[form] = (install, s[:ROWS], th[:ROWS], index[:ROWS], values[:ROWS])
    f = np.load(os.path.join(GOLDEN, "tabulated_grid_det.npz"))
    gamma, t, g, k = tg.fixture_set(1)              # set B: jittered nodes, pitch rows
    res["given nodes"] = (lambda ctx: ctx.set_tables_grid(gamma, t, g, k), f["s"][:ROWS].copy(), f["theta"][:ROWS].copy(),
                          f["index"][:ROWS].copy(), f["values"][1][:ROWS, :6].copy())
    return res


def clears(ctx):
    """the five entries with n_tables = 0, as a C caller reaches them -> their return codes when called"""
    lib, h, k = ctx.lib, ctx.handle, (ctypes.c_double * 1)(0.5)
    return (lambda: lib.rimphony_ctx_set_tables(h, 0, 0, 1.0, 2.0, None),
            lambda: lib.rimphony_ctx_set_tables_pitch(h, 0, 0, 1.0, 2.0, None, 0, None),
            lambda: lib.rimphony_ctx_set_tables_2d(h, 0, 0, 1.0, 2.0, 0, None),
            lambda: lib.rimphony_ctx_set_tables_pitchy(h, 0, 0, 1.0, 2.0, None, 0, None, k),
            lambda: lib.rimphony_ctx_set_tables_grid(h, 0, 0, None, None, 0, None, None))


@pytest.mark.parametrize("knob", [None, "0"], ids=["default routing", "RIMPHONY_TAB_GROUP=0"])
def test_every_form_after_every_other_and_every_clear(gpu_ctx, knob):
    """After each install of SEQUENCE the form's first four fixture rows, Symphony slots: the fixture's values bit for bit
    (NaN matching NaN) and the status words of the form's first computation on this context.  Then a set of each form in
    turn, cleared through each entry in turn: the kind is refused (RIMPHONY_EINVAL) and the next install computes the
    fixture's bits again."""
    from rimphony_amd import capi
    pairs = list(zip(SEQUENCE, SEQUENCE[1:]))
    assert len(pairs) == 20 and sorted(pairs) == [(a, b) for a in range(5) for b in range(5) if a != b]
    case = cases()
    first_status = {}

    def install_and_check(ctx, form, where):
        install, s, th, index, want = case[form]
        install(ctx)
        out, st = ctx.compute_batch(TAB, s, th, [index], MASK, want_status=True)
        assert same_bits(out[:, :6], want).all(), (where, form)
        assert np.isfinite(out[:, :6]).any(), (where, form)
        assert (st == first_status.setdefault(form, st)).all(), (where, form)

    with time_limit(300):
        gpu_ctx.shared_mode()           # (the session's context first: this one is in shared mode whatever test ran before)
        ctx = env_context() if knob is None else env_context(RIMPHONY_TAB_GROUP=knob)
        try:
            for n, i in enumerate(SEQUENCE):
                install_and_check(ctx, FORMS[i], "install %d" % n)
            for i, clear in enumerate(clears(ctx)):
                install_and_check(ctx, FORMS[i], "before clear %d" % i)
                assert clear() == 0, i
                _, s, th, index, _ = case[FORMS[i]]
                with pytest.raises(capi.RimphonyError, match="invalid argument"):
                    ctx.compute_batch(TAB, s, th, [index], MASK)
            install_and_check(ctx, FORMS[0], "after the last clear")
        finally:
            ctx.close()
