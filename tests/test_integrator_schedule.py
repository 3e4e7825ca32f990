"""The HMC integrator schedules on the host (include/dwhmc.h,
dwh_debug_integrator_schedule): the flattened (kick, drift) coefficients a
trajectory hands to the kick/drift kernels, from the function the enqueue
itself calls, and what the library refuses.  No device.

Comparisons are `==` on doubles: the leapfrog preset must form exactly the
doubles the trajectory formed before integrators were selectable (0.5*dt, dt,
dt/(2.0*mass)), and the presets' coefficients are products of two doubles, so
numpy forms the same bits.
"""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

LEAPFROG, OMELYAN2, CUSTOM = 0, 1, 2
LAM = 0.1931833275037836
ERR_ARG = -1


@pytest.fixture(scope="module")
def schedule(dwhmc):
    binding = import_module(dwhmc.__name__ + "._lib")
    lib = binding.load()

    def call(kind, Nt, dt, mass, lam=0.0, kick=None, drift=None, nstage=0):
        """(rc, kicks, drifts) straight from the ABI"""
        a = None if kick is None else np.ascontiguousarray(kick, dtype=np.float64)
        b = None if drift is None else np.ascontiguousarray(drift, dtype=np.float64)
        nfact = C.c_int64(-1)
        args = (kind, lam, nstage, binding.ptr(a), binding.ptr(b), Nt, dt, mass)
        rc = lib.dwh_debug_integrator_schedule(*args, C.byref(nfact), None, None)
        if rc != 0:
            assert lib.dwh_last_error(None), "a refusal names its reason"
            return rc, None, None
        n = nfact.value
        nk = n + 1 if n else 2
        kicks, drifts = np.full(nk + 1, np.nan), np.full(n + 1, np.nan)
        assert lib.dwh_debug_integrator_schedule(*args, C.byref(nfact), binding.ptr(kicks), binding.ptr(drifts)) == 0
        assert nfact.value == n
        assert np.isnan(kicks[nk]) and np.isnan(drifts[n]), "wrote past nfact + 1 kicks / nfact drifts"
        return 0, kicks[:nk], drifts[:n]

    return call


def test_leapfrog_is_todays_doubles(schedule):
    dt, m = 0.1, 1.3
    rc, kicks, drifts = schedule(LEAPFROG, 3, dt, m)
    assert rc == 0
    assert kicks.tolist() == [0.5 * dt, dt, dt, 0.5 * dt]
    assert drifts.tolist() == [dt / (2.0 * m)] * 3


def test_leapfrog_Nt0_two_half_kicks(schedule):
    dt = 0.1
    rc, kicks, drifts = schedule(LEAPFROG, 0, dt, 1.3)
    assert rc == 0
    assert kicks.tolist() == [0.5 * dt, 0.5 * dt] and len(drifts) == 0


@pytest.mark.parametrize("lam", [LAM, 0.18, 0.25])
def test_omelyan2_coefficients(schedule, lam):
    dt, m = 0.1, 1.3
    rc, kicks, drifts = schedule(OMELYAN2, 3, dt, m, lam=lam)
    assert rc == 0
    mid, two = (1.0 - 2.0 * lam) * dt, (lam + lam) * dt
    assert kicks.tolist() == [lam * dt, mid, two, mid, two, mid, lam * dt]
    assert drifts.tolist() == [0.5 * dt / (2.0 * m)] * 6


def test_custom_leapfrog_equals_leapfrog(schedule):
    for Nt, dt, m in [(3, 0.1, 1.3), (1, 0.37, 1.0), (7, 0.0123, 0.7)]:
        _, k0, d0 = schedule(LEAPFROG, Nt, dt, m)
        rc, k1, d1 = schedule(CUSTOM, Nt, dt, m, kick=[0.5, 0.5], drift=[1.0], nstage=1)
        assert rc == 0
        assert k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()


def test_custom_three_stage_merges_end_kicks(schedule):
    a, b = [0.1, 0.4, 0.4, 0.1], [0.25, 0.5, 0.25]
    dt, m = 0.2, 0.9
    rc, kicks, drifts = schedule(CUSTOM, 2, dt, m, kick=a, drift=b, nstage=3)
    assert rc == 0
    assert kicks.tolist() == [0.1 * dt, 0.4 * dt, 0.4 * dt, (0.1 + 0.1) * dt, 0.4 * dt, 0.4 * dt, 0.1 * dt]
    assert drifts.tolist() == [(x * dt) / (2.0 * m) for x in b + b]


def test_custom_omelyan_equals_preset(schedule):
    a = [LAM, 1.0 - 2.0 * LAM, LAM]
    _, k0, d0 = schedule(OMELYAN2, 4, 0.1, 1.3, lam=LAM)
    rc, k1, d1 = schedule(CUSTOM, 4, 0.1, 1.3, kick=a, drift=[0.5, 0.5], nstage=2)
    assert rc == 0 and k0.tobytes() == k1.tobytes() and d0.tobytes() == d1.tobytes()


@pytest.mark.parametrize("name,kw", [
    ("sum_a", dict(kick=[0.5, 0.5 + 1e-9], drift=[1.0], nstage=1)),
    ("sum_a_sym", dict(kick=[0.5 + 1e-9, 0.5 + 1e-9], drift=[1.0], nstage=1)),
    ("sum_b", dict(kick=[0.5, 0.5], drift=[1.0 - 1e-9], nstage=1)),
    ("sum_b_2", dict(kick=[0.25, 0.5, 0.25], drift=[0.5 + 0.5e-9, 0.5 + 0.5e-9], nstage=2)),
    ("not_palindromic_a", dict(kick=[0.2, 0.5, 0.3], drift=[0.5, 0.5], nstage=2)),
    ("not_palindromic_b", dict(kick=[0.25, 0.5, 0.25], drift=[0.4, 0.6], nstage=2)),
    ("not_palindromic_a_1ulp", dict(kick=[0.25, 0.5, np.nextafter(0.25, 1.0)], drift=[0.5, 0.5], nstage=2)),
    ("S0", dict(kick=[1.0], drift=[], nstage=0)),
    ("S17", dict(kick=[1.0 / 18] * 18, drift=[1.0 / 17] * 17, nstage=17)),
    ("S_negative", dict(kick=[0.5, 0.5], drift=[1.0], nstage=-1)),
    ("nan_a", dict(kick=[np.nan, np.nan], drift=[1.0], nstage=1)),
    ("nan_b", dict(kick=[0.5, 0.5], drift=[np.nan], nstage=1)),
    ("inf_a", dict(kick=[np.inf, -np.inf, 1.0, -np.inf, np.inf], drift=[0.25] * 4, nstage=4)),
    ("null_arrays", dict(kick=None, drift=None, nstage=1)),
    ("null_kick", dict(kick=None, drift=[1.0], nstage=1)),
    ("null_drift", dict(kick=[0.5, 0.5], drift=None, nstage=1)),
])
def test_custom_refused(schedule, name, kw):
    assert schedule(CUSTOM, 3, 0.1, 1.3, **kw)[0] == ERR_ARG


def test_custom_accepts_S16(schedule):
    a, b = [1.0 / 32] + [1.0 / 16] * 15 + [1.0 / 32], [1.0 / 16] * 16
    rc, kicks, drifts = schedule(CUSTOM, 2, 0.1, 1.0, kick=a, drift=b, nstage=16)
    assert rc == 0 and len(kicks) == 33 and len(drifts) == 32
    assert kicks[16] == (1.0 / 32 + 1.0 / 32) * 0.1


@pytest.mark.parametrize("lam", [0.0, 0.5, -0.1, np.nan])
def test_omelyan2_lambda_refused(schedule, lam):
    assert schedule(OMELYAN2, 3, 0.1, 1.3, lam=lam)[0] == ERR_ARG


def test_Nt0_only_for_leapfrog(schedule):
    assert schedule(OMELYAN2, 0, 0.1, 1.3, lam=LAM)[0] == ERR_ARG
    assert schedule(CUSTOM, 0, 0.1, 1.3, kick=[0.5, 0.5], drift=[1.0], nstage=1)[0] == ERR_ARG
    assert schedule(LEAPFROG, 0, 0.1, 1.3)[0] == 0


def test_bad_trajectory_arguments_refused(schedule):
    assert schedule(LEAPFROG, -1, 0.1, 1.3)[0] == ERR_ARG
    assert schedule(LEAPFROG, 3, 0.1, 0.0)[0] == ERR_ARG
    assert schedule(LEAPFROG, 3, np.inf, 1.3)[0] == ERR_ARG
    assert schedule(7, 3, 0.1, 1.3)[0] == ERR_ARG


def test_python_binding_matches_abi(dwhmc, schedule):
    """integrator_schedule (context.py) is the same call, names for codes and
    ValueError for DWH_ERR_ARG."""
    k, d = dwhmc.integrator_schedule("omelyan2", 3, 0.1, 1.3)
    _, k0, d0 = schedule(OMELYAN2, 3, 0.1, 1.3, lam=LAM)
    assert np.array_equal(k, k0) and np.array_equal(d, d0)
    assert dwhmc.OMELYAN2_LAMBDA == LAM
    k, d = dwhmc.integrator_schedule("custom", 2, 0.1, 1.0, kick=[0.5, 0.5], drift=[1.0])
    assert k.tolist() == [0.05, 0.1, 0.05]
    assert len(dwhmc.integrator_schedule("leapfrog", 0, 0.1, 1.0)[0]) == 2
    with pytest.raises(ValueError):
        dwhmc.integrator_schedule("omelyan2", 0, 0.1, 1.3)
    with pytest.raises(ValueError):
        dwhmc.integrator_schedule("custom", 2, 0.1, 1.0, kick=[0.4, 0.5], drift=[1.0])
    with pytest.raises(ValueError):
        dwhmc.integrator_schedule("rk4", 2, 0.1, 1.0)


def test_driver_option_parsing(dwhmc):
    """simulation.Integrator: names, dicts, Nt_min, and refusal before any file."""
    sim = import_module(dwhmc.__name__ + ".simulation")
    g = sim.Integrator("omelyan2")
    assert g.stages == 2 and g.Nt_min == 4 and g.args == {"kind": "omelyan2"}
    g = sim.Integrator(dict(kind="custom", kick=[0.25, 0.5, 0.25], drift=[0.5, 0.5], Nt_min=1))
    assert g.stages == 2 and g.Nt_min == 1
    assert sim.Integrator(dict(lam=0.2)).args == {"kind": "omelyan2", "lam": 0.2}
    assert sim.parse_integrator(None) is None
    for bad in (dict(kind="omelyan2", lam=0.5), dict(kind="omelyan2", Nt_min=0), dict(step=3), "verlet",
                dict(kind="custom", kick=[0.3, 0.5, 0.2], drift=[0.5, 0.5])):
        with pytest.raises(ValueError):
            sim.Integrator(bad)
    ctl = sim.AdaptiveNt(3, Nt_min=1)
    for i in range(1, 11):
        ctl.record(i, True)
    assert ctl.Nt == 1
    ctl = sim.AdaptiveNt(5)
    for i in range(1, 11):
        ctl.record(i, True)
    assert ctl.Nt == 4
