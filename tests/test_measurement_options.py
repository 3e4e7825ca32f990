"""The five measurement options of the drivers (simulation.OPTIONS:
spectral_maps, current_response, operator_response, nambu_response,
response_map) go through one pipeline; these tests pin what that pipeline must
keep, on the oracle backend with all five mixins on one context (CPU only):

1. a run with all five options writes, file by file and array by array, what
   the five runs with one option each write (bytes; simulation.log apart), its
   file list is their union and its bins hold the keys in the fixed order;
2. the device call pattern: one measure_transport_deltas and one call of each
   option per flush with the whole batch's Δ; at transport_batch 1 calls at
   the device Δ (deltas=None), for chains one measure_transport_all per
   measurement and never a per-chain measure_transport;
3. the parsed defaults of each option, and a TransportQueue built from raw
   dicts against one handed the parsed options.
"""
import importlib
import os

import numpy as np
import pytest

from nambu_reference import OracleNambu
from oracle_measurements import OracleMaps, OracleOperator, OracleResponse, simulate
from response_map_reference import OracleMap
from test_current_response import SIM_KW, SIM_OPT as OPT_CURRENT
from test_nambu_response import SIM_OPT as OPT_NAMBU
from test_operator_response import SIM_OPT as OPT_OPERATOR
from test_response_map import SIM_OPT as OPT_MAP
from test_spectral_maps import SIM_WIN

OPTS = dict(spectral_maps=SIM_WIN, current_response=OPT_CURRENT, operator_response=OPT_OPERATOR,
            nambu_response=OPT_NAMBU, response_map=OPT_MAP)
BIN_KEYS = ["opt_cond", "dos", "dos_AN", "A_k0", "count", "ldos", "akw", "chi2", "nambu_chi2", "response_map",
            "rho_map"]
CASES = [(0, 1), (0, 3), (2, 1), (2, 2)]          # (chains, transport_batch)
MEASURES = ["measure_spectral_maps", "measure_current_response", "measure_operator_response",
            "measure_nambu_response", "measure_response_map"]


class OracleAll(OracleMaps, OracleResponse, OracleOperator, OracleNambu, OracleMap):
    """the oracle backend with every measure_* call"""


def _counting(log):
    """OracleAll whose measure_* calls append (name, nstates or None, chain) to log: the
    drivers' calls, not those the oracle backend makes of itself inside one
    (its measure_transport_deltas and measure_transport_all loop over measure_transport)"""
    def wrap(name):
        def call(self, *a, **kw):
            if getattr(self, "_inside", False):
                return getattr(super(Counting, self), name)(*a, **kw)
            deltas = a[0] if name == "measure_transport_deltas" else kw.get("deltas")
            log.append((name, None if deltas is None else len(deltas), kw.get("chain")))
            self._inside = True
            try:
                return getattr(super(Counting, self), name)(*a, **kw)
            finally:
                self._inside = False
        return call
    Counting = type("Counting", (OracleAll,), {})
    for name in MEASURES + ["measure_transport", "measure_transport_deltas", "measure_transport_all"]:
        setattr(Counting, name, wrap(name))
    return Counting


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def trees(dwhmc, tmp_path_factory):
    """{(chains, tb): (all-options directory, {keyword: its single-option directory})}, each run once"""
    root = tmp_path_factory.mktemp("options")
    out = {}
    for chains, tb in CASES:
        d = root / f"all_{chains}_{tb}"
        simulate(dwhmc, d, OracleAll, chains=chains, transport_batch=tb, **OPTS, **SIM_KW)
        single = {}
        for k, v in OPTS.items():
            single[k] = root / f"{k}_{chains}_{tb}"
            simulate(dwhmc, single[k], OracleAll, chains=chains, transport_batch=tb, **{k: v}, **SIM_KW)
        out[chains, tb] = (d, single)
    return out


@pytest.mark.parametrize("chains,tb", CASES)
def test_all_options_equal_each_option_alone(trees, chains, tb):
    both, single = trees[chains, tb]
    union = set()
    for k, d in single.items():
        for f in _files(d):
            union.add(f)
            if f.endswith("simulation.log"):
                continue
            assert f in _files(both), (k, f)
            if f.endswith(".npz"):
                a, b = np.load(both / f), np.load(d / f)
                for name in b.files:
                    assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (k, f, name)
            else:
                assert (both / f).read_bytes() == (d / f).read_bytes(), (k, f)
    assert _files(both) == sorted(union)
    bins = [f for f in _files(both) if f.endswith(".npz")]
    assert len(bins) == max(chains, 1) * SIM_KW["n_measure"] // SIM_KW["bin_size"]
    for f in bins:
        assert np.load(both / f).files == BIN_KEYS, f
    for sub in ([f"c{c}" for c in range(chains)] or ["."]):
        assert sorted(f for f in os.listdir(both / sub) if f.endswith(".csv")) == [
            "current_response.csv", "nambu_response.csv", "observables.csv", "operator_response.csv", "transport.csv"]
        assert sorted(f for f in os.listdir(both / sub / "spectra_bins") if f.endswith(".npy")) == [
            "chi2_omega.npy", "maps_omega.npy", "nambu_chi2_omega.npy", "omega_grid.npy", "response_map_pattern.npy"]


def _calls(dwhmc, tmp_path, chains, tb):
    log = []
    simulate(dwhmc, tmp_path, _counting(log), chains=chains, transport_batch=tb, **OPTS, **SIM_KW)
    return {name: [(ns, ch) for n, ns, ch in log if n == name] for name in {n for n, _, _ in log}}


def test_call_pattern_batched_queue(dwhmc, tmp_path):
    """n_measure = 4 at transport_batch = 3: two flushes, of 3 and of 1 states."""
    calls = _calls(dwhmc, tmp_path, 0, 3)
    assert sorted(calls) == sorted(MEASURES + ["measure_transport_deltas"])
    for name, got in calls.items():
        assert got == [(3, 0), (1, 0)], (name, got)


def test_call_pattern_single_chain_unbatched(dwhmc, tmp_path):
    calls = _calls(dwhmc, tmp_path, 0, 1)
    assert sorted(calls) == sorted(MEASURES + ["measure_transport"])
    for name, got in calls.items():
        assert got == [(None, 0)] * 4, (name, got)


def test_call_pattern_chains_unbatched(dwhmc, tmp_path):
    """transport for all chains in one measure_transport_all per measurement
    (the batched eigensolve), the options chain by chain at the device Δ."""
    calls = _calls(dwhmc, tmp_path, 2, 1)
    assert sorted(calls) == sorted(MEASURES + ["measure_transport_all"])
    assert calls["measure_transport_all"] == [(None, None)] * 4
    for name in MEASURES:
        assert calls[name] == [(None, 0), (None, 1)] * 4, (name, calls[name])


@pytest.fixture(scope="module")
def sim(dwhmc):
    return importlib.import_module(dwhmc.__name__ + ".simulation")


def _model(dwhmc):
    return dwhmc.ModelParameters(4, 4, 1.0, -0.35, -1.08, 1.0, 0.25, 8.0, 0.8, 1.0)


def test_option_order_and_parsed_defaults(dwhmc, sim):
    p = _model(dwhmc)
    VX = importlib.import_module(dwhmc.__name__ + ".vertices")
    assert [o.keyword for o in sim.OPTIONS] == list(OPTS)
    assert sim.parse_options(p) == [] and sim.parse_options(p, **dict.fromkeys(OPTS)) == []
    maps, cur, oper, nam, rmap = sim.parse_options(p, **{k: {} for k in OPTS})
    assert maps.window == dict(first=0, count=None, stride=1)
    assert np.array_equal(maps.header[1], dwhmc.spectral_window(p.eta, p.domega, p.omega_max))
    assert cur.args == dict(direction="x", q=[(0, 1)], n_matsubara=1)
    assert oper.names == [("density", (0, 0))] and oper.spin_sign == [VX.build("density", p, 0, 0).spin_sign]
    assert nam.names == [("pair_d_create", (0, 0))] and nam.pairs == [(0, 0)]
    assert rmap.names == [("current_x", (0, 0))] and rmap.omega is None
    assert rmap.pattern.dtype == np.int64 and np.array_equal(rmap.pattern, VX.bond_pattern(p))
    for o in (oper, nam, rmap):
        assert (o.n_matsubara, o.omega, o.eta) == (1, None, p.eta)
    assert [o.header and o.header[0] for o in (maps, cur, oper, nam, rmap)] == [
        "maps_omega.npy", None, None, None, "response_map_pattern.npy"]
    assert [o.csv_file for o in (maps, cur, oper, nam, rmap)] == [
        None, "current_response.csv", "operator_response.csv", "nambu_response.csv", None]
    # the grids' header files and the CSV files follow omega and n_matsubara
    grid = dict(start=-0.2, step=0.2, count=3)
    oper, nam = sim.parse_options(p, operator_response=dict(omega=grid, n_matsubara=0),
                                  nambu_response=dict(omega=grid, n_matsubara=0, eta=0.3))
    assert (oper.header[0], nam.header[0]) == ("chi2_omega.npy", "nambu_chi2_omega.npy")
    assert oper.omega == nam.omega == (-0.2, 0.2, 3) and (oper.eta, nam.eta) == (p.eta, 0.3)
    assert np.array_equal(oper.header[1], -0.2 + 0.2 * np.arange(3)) and oper.csv_file is None and nam.csv_file is None


@pytest.mark.parametrize("bad", [
    dict(spectral_maps=dict(step=2)), dict(spectral_maps=dict(first=4001)), dict(current_response=dict(nq=2)),
    dict(operator_response=dict(ops=[])), dict(operator_response=dict(n_matsubara=0)),
    dict(operator_response=dict(omega=dict(start=0.0, step=0.1))), dict(nambu_response=dict(vertices=[])),
    dict(nambu_response=dict(pairs=[(0, 1)])), dict(nambu_response=dict(omega=dict(start=0.0, step=0.1, n=3))),
    dict(nambu_response=dict(n_matsubara=-1)), dict(response_map=dict(pattern=dict(range=("site",)))),
    dict(response_map=dict(pattern=np.zeros((0, 2), dtype=np.int64))), dict(response_map=dict(pattern=[[0, 32]])),
    dict(response_map=dict(n_matsubara=0, omega=[]))])
def test_bad_options_raise_before_any_file_is_opened(dwhmc, sim, tmp_path, bad):
    with pytest.raises(ValueError):
        sim.parse_options(_model(dwhmc), **bad)
    for chains in (0, 2):
        with pytest.raises(ValueError):
            simulate(dwhmc, tmp_path / f"run{chains}", OracleAll, chains=chains, **bad, **SIM_KW)
    assert os.listdir(tmp_path) == []


def test_shared_intake_of_the_binding(dwhmc):
    """FermionContext's shared argument intake (no device): the ABI layout of
    deltas and the one place that accepts no states, the omega grid forms, the
    CSR tuple with each caller's message, the state axis of the results."""
    import types
    C = importlib.import_module(dwhmc.__name__ + ".context")
    me = types.SimpleNamespace(N=3)
    states = C.FermionContext._states
    D = np.arange(12, dtype=np.float64).reshape(2, 3, 2) * (1 + 1j)
    ns, d = states(me, D)
    assert ns == 2 and d.shape == (2, 2, 3) and d.flags["C_CONTIGUOUS"] and np.array_equal(d, D.transpose(0, 2, 1))
    assert states(me, None) == (1, None)
    assert states(me, np.zeros((0, 3, 2)), min_states=0)[0] == 0
    for bad, kw in ((np.zeros((3, 2)), {}), (np.zeros((2, 4, 2)), {}), (np.zeros((0, 3, 2)), {}),
                    (None, dict(min_states=0)), (np.zeros((3, 2)), dict(min_states=0))):
        with pytest.raises(ValueError, match=r"expected \(nstates, 3, 2\) pairing fields"):
            states(me, bad, **kw)
    assert C._omega_grid(None, None) == (0.0, 0.0, 0)
    assert C._omega_grid(dict(start=-1, step=0.5, count=4), 0.1) == C._omega_grid((-1, 0.5, 4.0), 0.1) == (-1.0, 0.5, 4)
    with pytest.raises(ValueError, match=r"omega: unknown keys \['n'\]"):
        C._omega_grid(dict(start=0, step=1, n=2), 0.1)
    with pytest.raises(ValueError, match="eta is needed with omega"):
        C._omega_grid((0, 1, 2), None)
    rowptr, col, val = C._csr_tuple(([0, 1, 2, 2], np.array([2, 0], dtype=np.int32), [1.0, 2j]), 3, "m")
    assert (rowptr.dtype, col.dtype, val.dtype) == (np.int64, np.int64, np.complex128) and val.shape == (1, 2)
    with pytest.raises(ValueError, match=r"^rowptr of 4 and val \(nops, 2\)$"):
        C._csr_tuple(([0, 1, 2], [2, 0], [[1.0, 2.0]]), 3, "rowptr of {n} and val (nops, {nnz})")
    with pytest.raises(ValueError, match=r"^val \(nops, 2\)$"):
        C._csr_tuple(([0, 1, 2, 2], [2, 0], [[1.0, 2.0, 3.0]]), 3, "val (nops, {nnz})")
    a, s = np.arange(6.0).reshape(2, 3), np.array([4.0, 5.0])
    all_states = C._per_state(D, scalars=("s",), a=a, s=s, n=None)
    assert list(all_states) == ["a", "s", "n"] and all_states["a"] is a and all_states["s"] is s
    one = C._per_state(None, scalars=("s",), a=a, s=s, n=None)
    assert np.array_equal(one["a"], a[0]) and one["s"] == 4.0 and type(one["s"]) is float and one["n"] is None


def test_queue_from_raw_dicts_equals_queue_with_parsed_options(dwhmc, sim, tmp_path):
    p = _model(dwhmc)
    rng = np.random.default_rng(5)
    ctx = OracleAll(p.Lx, p.Ly, p.t, p.tp, p.mu, p.beta, p.J, p.nn_table, p.nnn_table, rng.standard_normal(p.N))
    fields = 0.3 * (rng.standard_normal((3, p.N, 2)) + 1j * rng.standard_normal((3, p.N, 2)))

    def run(d, make):
        out, res = sim.ChainOutput(str(d), False), sim.SimulationResult(0, 0.0, 0.0)
        try:
            tq = make(ctx, p, out, res, 2, 2)
            sim.write_headers(out.spec_dir, p, tq.options)
            for i, D in enumerate(fields):
                tq.add(i + 1, D)
            tq.flush()
        finally:
            out.close()
        assert [i for i, _ in res.transport] == [1, 2, 3]

    run(tmp_path / "raw", lambda *a: sim.TransportQueue(*a, **OPTS))
    options = sim.parse_options(p, **OPTS)
    run(tmp_path / "parsed", lambda *a: sim.TransportQueue.with_options(options, *a))
    files = _files(tmp_path / "raw")
    assert files == _files(tmp_path / "parsed") and "spectra_bins/sweep_2.npz" in files
    assert {"current_response.csv", "operator_response.csv", "nambu_response.csv"} <= set(files)
    for f in files:
        if f.endswith(".npz"):                                # (a zip: its bytes carry the time of writing)
            a, b = np.load(tmp_path / "raw" / f), np.load(tmp_path / "parsed" / f)
            assert a.files == b.files == BIN_KEYS and all(a[k].tobytes() == b[k].tobytes() for k in BIN_KEYS), f
        elif not f.endswith("simulation.log"):
            assert (tmp_path / "raw" / f).read_bytes() == (tmp_path / "parsed" / f).read_bytes(), f
