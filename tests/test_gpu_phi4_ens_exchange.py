"""Replica exchange of the phi^4 ensemble on the GPU (sq_phi4_ens_exchange, sq_phi4_ens_step_hmc_exchange) against
the NumPy statement of the header's definition (phi4_exchange_model.py): the pairing, u from oracle.philox, Δ from
the slots' float records and `moments()` of the fields they hold, the verdict from the kernel's own Δ and u.

Tolerances.  u, partners, walkers, fields, counters: exact.  Δ against the model: 1e-10 A, A the sum of the
magnitudes of its three products (the kernel and the model form them from the same doubles; they may round the
coefficients' quotients differently by an ulp or two, 2e-16 A each).  A pair with |exp(-Δ) - u| < 1e-12 cannot be
decided across two exp implementations and is left out of the verdict check; at most 1 % of the pairs may be.  The
physics test's bounds are derived at the test."""
import numpy as np
import pytest

import phi4_exchange_model as xm
from test_gpu_phi4_ens_heun import CLAMP, _free_phi2
from test_gpu_phi4_ens_hmc import CLASS_SHAPES
from test_gpu_phi4_ens_hmc import _dtau as _hmc_dtau
from test_gpu_phi4_ens_mala import THERM, _record
from test_oracle import same_bits
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
LADDER = (1.0, 1.07, 1.145, 1.225)      # C per rung
M2, LAM, DTAU = 0.5, 1.0, 0.01
ROUNDS = (7, 2 ** 40 + 5)               # both parities within exchange(2), and the high counter word
SEED0 = 0xC0FFEE

_seen = {}                              # shape -> the verdicts of the oracle test


def _seeds(R, base=SEED0):
    return [base + 0x9E3779B97F4A7C15 * (r + 1) & (2 ** 64 - 1) for r in range(R)]


def _ens(shape, R=8, C=None, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU)
    kw.setdefault("m2", M2)
    kw.setdefault("lam", LAM)
    kw.setdefault("seeds", _seeds(R))
    kw.setdefault("clamp", CLAMP)
    return Phi4Ensemble(shape, R, C=list(np.resize(LADDER, R)) if C is None else C, **kw)


def _records(E):
    p = E.get_params()
    return [_record(p["dtau"][r], p["m2"][r], p["lam"][r], p["C"][r]) for r in range(E.R)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_rounds(o, E, seeds, nrounds):
    """Run exchange(nrounds, record=True) on E and check every row of the record, the fields, the labels and the
    counters against the model, from the state E is in.  Returns (verdicts of all pairs, pairs left undecided)."""
    R, nlad, x0 = E.R, E.ladder, E.exchange_round
    recs = _records(E)
    start, mom = E.download(), E.moments()
    mom = np.stack([mom[k] for k in ("S1", "S2", "S4", "NN", "maxabs")], axis=1)      # rows as the C call's
    held = list(range(R))                       # held[r]: the row of `start` that slot r holds
    lab = [int(w) for w in E.walkers()]
    stats = E.exchange_stats().copy()
    launches = E.perf()["kernel_launches"]
    rec = E.exchange(nrounds, record=True)
    assert rec.shape == (nrounds, R, 5)
    verdicts, skipped = [], 0
    for i in range(nrounds):
        x = x0 + i
        part = xm.partners(R, nlad, x)
        assert [int(v) for v in rec[i, :, 3]] == part, (x, rec[i, :, 3])
        for a, b in xm.pairs(R, nlad, x):
            d, u, v = (float(t) for t in rec[i, a, :3])
            assert np.array_equal(_bits(rec[i, a, :3]), _bits(rec[i, b, :3])), (x, a)
            assert u == xm.uniform(o, seeds[a], x), (x, a, u)
            ref, A = xm.delta(recs[a], recs[b], mom[held[a]], mom[held[b]])
            assert abs(d - ref) <= 1e-10 * A, (x, a, d, ref, A)
            with np.errstate(over="ignore"):
                e = float(np.exp(-d))
            if d > 0.0 and abs(e - u) < 1e-12:
                skipped += 1
            else:
                assert v == float(xm.verdict(d, u)), (x, a, d, u, v)
            stats[a, 0] += 1
            stats[a, 1] += int(v)
            if v == 1.0:
                held[a], held[b] = held[b], held[a]
                lab[a], lab[b] = lab[b], lab[a]
            verdicts.append(int(v))
        for r in range(R):
            if part[r] < 0:
                assert list(rec[i, r, :3]) == [0.0, 0.0, -1.0], (x, r, rec[i, r])
        assert [int(w) for w in rec[i, :, 4]] == lab, (x, rec[i, :, 4], lab)
    assert same_bits(E.download(), start[held]), "rows after the rounds"
    assert [int(w) for w in E.walkers()] == lab
    assert np.array_equal(E.exchange_stats(), stats)
    assert E.exchange_round == x0 + nrounds
    assert E.perf()["kernel_launches"] == launches + sum(1 for i in range(nrounds) if xm.pairs(R, nlad, x0 + i)), \
        "one launch per round with a pair"
    return verdicts, skipped


def _run_shape(o, shape):
    if shape in _seen:
        return _seen[shape]
    assert_shape(shape)
    seeds = _seeds(8)
    with _ens(shape) as E:
        assert E.ladder == 0 and E.exchange_round == 0
        assert list(E.walkers()) == list(range(8)) and not E.exchange_stats().any()
        E.set_ladder(4)
        assert E.ladder == 4
        E.init_field(0.5)
        E.step(THERM)
        steps, flags, params = list(E.step_counter), list(E.flags()), E.get_params()
        verdicts, skipped = [], 0
        for x in ROUNDS:
            E.exchange_round = x
            v, s = check_rounds(o, E, seeds, 2)
            verdicts += v
            skipped += s
        assert list(E.step_counter) == steps and list(E.flags()) == flags
        assert all(np.array_equal(E.get_params()[k], params[k]) for k in params)
    assert len(verdicts) == 2 * (4 + 2) and skipped <= 0.01 * len(verdicts), (shape, skipped)
    print(f"exchange {shape} verdicts {verdicts}", flush=True)
    _seen[shape] = verdicts
    return verdicts


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_model(gpu, dev_oracle, shape):
    _run_shape(dev_oracle, shape)


def test_both_verdicts_occur_over_the_shapes(gpu, dev_oracle):
    vs = [v for shape in SHAPES for v in _run_shape(dev_oracle, shape)]
    assert 0 in vs and 1 in vs, vs


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_each_verdict_in_every_class(gpu, dev_oracle, shape):
    """Uploaded fields: in pair (0, 1) the hot slot holds the low-energy field (Δ < 0: accepted), in pair (2, 3) the
    cold one does (Δ >> 0: exp(-Δ) is below the smallest u, 2^-33)."""
    assert_shape(shape)
    assert {GPU_SHAPES[s][0::2] for s in CLASS_SHAPES} == {GPU_SHAPES[s][0::2] for s in GPU_SHAPES}
    rng = np.random.default_rng(5)
    ls = (shape[2], shape[1], shape[0])
    big, small = (rng.normal(0.0, s, (2,) + ls).astype(np.float32) for s in (1.0, 0.1))
    seeds = _seeds(4)
    with _ens(shape, R=4, C=[1.0, 1.225, 1.0, 1.225]) as E:
        E.set_ladder(2)
        E.upload(np.stack([big[0], small[0], small[1], big[1]]))
        E.exchange_round = 2 ** 33 + 2
        verdicts, skipped = check_rounds(dev_oracle, E, seeds, 1)
        assert verdicts == [1, 0] and skipped == 0
        got = E.download()
        assert same_bits(got, np.stack([small[0], big[0], small[1], big[1]]))
        assert list(E.walkers()) == [1, 0, 2, 3]
        assert E.exchange_stats().tolist() == [[1, 1], [0, 0], [1, 0], [0, 0]]


def _state(E):
    G, S1, n = E.corr_sums()
    p = E.perf()
    return {"field": E.download().view(np.uint32), "steps": np.asarray(E.step_counter), "flags": np.asarray(E.flags()),
            "hmc": E.hmc_stats(), "mala": E.mala_stats(), "xstat": E.exchange_stats(), "walkers": E.walkers(),
            "round": np.asarray(E.exchange_round), "G": _bits(G), "S1": _bits(S1), "nmeas": np.asarray(n),
            "perf": np.asarray([p["steps"], p["kernel_launches"]])}


def _same_state(A, B):
    a, b = _state(A), _state(B)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _thermal(shape, R=8, **kw):
    E = _ens(shape, R=R, dtau=_hmc_dtau(shape), **kw)
    E.init_field(0.5)
    E.step(THERM)
    E.set_ladder(4)
    return E


@pytest.mark.parametrize("shape", [(8, 8, 8), (16, 24, 24), (32, 32, 32)])
def test_fused_call_is_the_loop(gpu, shape):
    assert_shape(shape)
    with _thermal(shape) as A, _thermal(shape) as B:
        ser, rh, rx = A.step_hmc_exchange(6, ntraj=2, nleap=3, randomize=True, every=1, correlate=True, record=True)
        assert ser.shape == (12, 8, 4) and rh.shape == (12, 8, 4) and rx.shape == (6, 8, 5)
        parts = []
        for _ in range(6):
            s, r = B.step_hmc(2, nleap=3, randomize=True, every=1, correlate=True, record=True)
            parts.append((s, r, B.exchange(1, record=True)))
        for got, k in ((ser, 0), (rh, 1), (rx, 2)):
            assert np.array_equal(_bits(got), _bits(np.concatenate([p[k] for p in parts]))), k
        _same_state(A, B)
        assert A.exchange_round == 6 and A.perf()["kernel_launches"] == B.perf()["kernel_launches"]
        assert set(rx[:, :, 2].ravel()) <= {-1.0, 0.0, 1.0} and (rh[:, :, 2] == 1.0).any()
        # without records and measurements: the same fields, counters and labels
        with _thermal(shape) as C:
            assert C.step_hmc_exchange(6, ntraj=2, nleap=3, randomize=True) is None
            assert same_bits(C.download(), A.download())
            assert np.array_equal(C.walkers(), A.walkers()) and np.array_equal(C.exchange_stats(), A.exchange_stats())
            assert np.array_equal(C.hmc_stats(), A.hmc_stats()) and list(C.step_counter) == list(A.step_counter)


def test_a_ladder_does_not_depend_on_its_neighbours(gpu):
    shape = (8, 8, 8)
    seeds = _seeds(16)
    with _thermal(shape, R=16) as A, _thermal(shape, R=4, seeds=seeds[12:]) as B:
        sa, ha, xa = A.step_hmc_exchange(5, ntraj=2, nleap=2, every=2, record=True)
        sb, hb, xb = B.step_hmc_exchange(5, ntraj=2, nleap=2, every=2, record=True)
        assert np.array_equal(_bits(sa[:, 12:]), _bits(sb)) and np.array_equal(_bits(ha[:, 12:]), _bits(hb))
        assert np.array_equal(_bits(xa[:, 12:, :3]), _bits(xb[:, :, :3]))
        off = np.where(xb[:, :, 3:] >= 0, 12.0, 0.0)
        assert np.array_equal(xa[:, 12:, 3:], xb[:, :, 3:] + off)
        assert same_bits(A.download(12, 4), B.download())
        assert np.array_equal(A.walkers(12, 4), B.walkers() + 12)
        assert np.array_equal(A.exchange_stats(12, 4), B.exchange_stats())
        assert (xa[:, :, 2] == 1.0).any()


def test_rounds_split_over_calls(gpu):
    shape = (8, 8, 8)
    with _thermal(shape) as A, _thermal(shape) as B:
        for E in (A, B):
            E.step_hmc(4, nleap=3)
            E.exchange_round = 2 ** 32 - 2        # the low word wraps inside the call
        ra = A.exchange(4, record=True)
        rb = np.concatenate([B.exchange(1, record=True) for _ in range(4)])
        assert np.array_equal(_bits(ra), _bits(rb))
        _same_state(A, B)
        assert A.exchange(0) is None and A.exchange(0, record=True).shape == (0, 8, 5)
        assert A.exchange_round == 2 ** 32 + 2


def test_a_round_without_a_pair_changes_only_the_counter(gpu):
    shape = (8, 8, 8)
    with _thermal(shape) as E:
        E.set_ladder(2)
        E.exchange(2)                             # rounds 0 (four pairs) and 1 (none)
        assert E.exchange_round == 2 and E.exchange_stats()[:, 0].tolist() == [1, 0] * 4
        E.exchange_round = 5
        before = _state(E)
        rec = E.exchange(1, record=True)
        after = _state(E)
        assert rec[0, :, :4].tolist() == [[0.0, 0.0, -1.0, -1.0]] * 8
        assert rec[0, :, 4].tolist() == [float(w) for w in before["walkers"]]
        assert after.pop("round") == 6 and before.pop("round") == 5
        for k in before:
            assert np.array_equal(before[k], after[k]), k


@pytest.mark.parametrize("nlad", [3, 5])
def test_odd_ladders_pair_as_the_table_says(gpu, dev_oracle, nlad):
    shape = (8, 8, 8)
    R = 2 * nlad
    seeds = _seeds(R)
    with _ens(shape, R=R, C=list(np.resize(LADDER + (1.31,), R))) as E:
        E.init_field(0.5)
        E.step(THERM)
        E.set_ladder(nlad)
        check_rounds(dev_oracle, E, seeds, 4)
        assert E.exchange_stats()[:, 0].tolist() == ([2, 2, 0] if nlad == 3 else [2, 2, 2, 2, 0]) * 2


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_site_rejects(gpu, bad):
    """NaN: the sums are NaN, so is Δ.  +inf among positive neighbours: S2 and NN are +inf, the first two products
    are infinities of one sign and their difference is NaN.  Verdict 0, both rows keep their bits."""
    shape = (16, 4, 31)
    rng = np.random.default_rng(3)
    f = np.abs(rng.normal(0.0, 0.5, (2, 31, 4, 16))).astype(np.float32) + np.float32(0.01)
    for slot in (0, 1):
        g = f.copy()
        g[slot, 17, 2, 5] = bad
        with _ens(shape, R=2, C=[1.0, 1.07]) as E:
            E.set_ladder(2)
            E.upload(g)
            rec = E.exchange(1, record=True)
            assert np.isnan(rec[0, 0, 0]) and rec[0, :, 2].tolist() == [0.0, 0.0], rec
            assert same_bits(E.download(), g)
            assert E.exchange_stats().tolist() == [[1, 0], [0, 0]] and list(E.walkers()) == [0, 1]
            assert not E.flags().any()


def test_equal_parameters_always_accept(gpu):
    shape = (8, 17, 31)
    with _ens(shape, R=4, C=[1.1] * 4) as E:
        E.init_field(0.7)
        E.set_ladder(4)
        start = E.download()
        rec = E.exchange(6, record=True)
        paired = rec[:, :, 3] >= 0
        assert (rec[:, :, 0][paired] == 0.0).all() and (rec[:, :, 2][paired] == 1.0).all()
        st = E.exchange_stats()
        assert st.tolist() == [[3, 3], [3, 3], [3, 3], [0, 0]]
        # six rounds of always-accepted swaps on four slots: an odd-even transposition sort run backwards
        w = list(E.walkers())
        assert sorted(w) == [0, 1, 2, 3] and w != [0, 1, 2, 3]
        assert same_bits(E.download(), start[w])


def test_exchange_reset(gpu):
    shape = (8, 8, 8)
    with _ens(shape, R=8, C=[1.0] * 8) as E:
        E.init_field(0.5)
        E.set_ladder(4)
        E.exchange(3)
        st, w = E.exchange_stats(), list(E.walkers())
        assert st[:, 0].sum() == 10 and w != list(range(8))
        E.exchange_reset(first=4, count=4)
        assert np.array_equal(E.exchange_stats(0, 4), st[:4]) and not E.exchange_stats(4).any()
        assert list(E.walkers()) == w and E.exchange_round == 3
        E.exchange_reset(first=0, count=4, walkers=True)
        assert not E.exchange_stats().any() and list(E.walkers()) == [0, 1, 2, 3] + w[4:]
        E.exchange_reset(walkers=True)
        assert list(E.walkers()) == list(range(8))


def test_state_and_argument_errors_launch_nothing(gpu):
    from stochquant_amd import StochQuantError
    shape = (8, 8, 8)
    with _ens(shape, R=6, C=[1.0, 1.07, 1.145] * 2) as E:
        E.init_field(0.5)
        for nlad in (1, 4, 5, 7, 12, -2):
            with pytest.raises(StochQuantError) as ei:
                E.set_ladder(nlad)
            assert ei.value.code == -1 and E.ladder == 0
        before = _state(E)

        def refused(code):
            for call in (lambda: E.exchange(2), lambda: E.exchange(0), lambda: E.exchange(1, record=True),
                         lambda: E.step_hmc_exchange(2, ntraj=2, nleap=2),
                         lambda: E.step_hmc_exchange(0)):
                with pytest.raises(StochQuantError) as ei:
                    call()
                assert ei.value.code == code
            after = _state(E)
            for k in before:
                assert np.array_equal(before[k], after[k]), k

        refused(-4)                               # no ladder: SQ_E_STATE
        E.set_ladder(3)
        E.set_params(C=0.0, first=4, count=1)
        refused(-4)                               # a C = 0 replica: SQ_E_STATE
        E.set_params(C=1.07, first=4, count=1)
        E.set_ladder(0)
        assert E.ladder == 0
        refused(-4)


def test_c_call_argument_errors(gpu, sqlib):
    """The C call's own checks, where the Python wrapper would raise first: ntraj % every, nleap, negative counts."""
    with _thermal((8, 8, 8)) as E:
        before = _state(E)
        for args in ((2, 3, 1, 0, 2, None, 0, None, None), (2, 2, 0, 0, 0, None, 0, None, None),
                     (-1, 2, 1, 0, 0, None, 0, None, None), (2, -1, 1, 0, 0, None, 0, None, None),
                     (2, 2, 1, 0, 0, None, 1, None, None), (2, 2, 1, 0, 0, None, 2, None, None)):
            assert sqlib.sq_phi4_ens_step_hmc_exchange(E._h, *args) == -1, args
        assert sqlib.sq_phi4_ens_exchange(E._h, -1, None) == -1
        after = _state(E)
        for k in before:
            assert np.array_equal(before[k], after[k]), k


def test_detailed_balance_on_the_free_field(gpu):
    """The free field (λ = 0, m² = 1) on 8 x 4 x 4, 64 ladders of four rungs.  Rung i samples exp(-S / C_i²): <φ²>
    per site is C_i² times the exact lattice value, and S is C_i² χ²_128 / 2.  An exchange rule that broke detailed
    balance would mix rungs whose <φ²> differ by 14 %.  Every bound is five standard errors, the errors from the
    scatter of the 64 ladders' time means, and the errors themselves are bounded so that noise cannot pass."""
    shape, V, NL, NR = (8, 4, 4), 128, 64, 2000
    exact = _free_phi2(shape, 1.0, 0.02)["continuum"]
    assert abs(exact - 0.1727010510) < 1e-9
    C = np.asarray(LADDER)
    with _ens(shape, R=4 * NL, C=list(np.tile(C, NL)), dtau=0.02, m2=1.0, lam=0.0, seeds=_seeds(4 * NL, 77)) as E:
        E.set_ladder(4)
        E.init_field(0.4)
        E.step(500, scheme="heun")
        E.step_hmc_exchange(200, ntraj=2, nleap=4, randomize=True)
        E.exchange_reset(walkers=True)
        E.hmc_reset()
        s2 = np.zeros(4 * NL)
        em = np.zeros(NL)
        npair = 0
        visited = np.zeros((4 * NL, 4), dtype=bool)      # [walker][rung]
        visited[np.arange(4 * NL), np.arange(4 * NL) % 4] = True
        for _ in range(4):
            ser, _, rx = E.step_hmc_exchange(NR // 4, ntraj=2, nleap=4, randomize=True, every=2, record=True)
            s2 += ser[:, :, 1].sum(axis=0)
            low = (rx[:, :, 3] > np.arange(4 * NL)[None, :])          # the lower slot of every pair
            ex = np.where(low, np.exp(-rx[:, :, 0]), 0.0)
            em += ex.sum(axis=0).reshape(NL, 4).sum(axis=1)
            npair += int(low.sum())
            w = rx[:, :, 4].astype(int)
            visited[w, np.arange(4 * NL)[None, :] % 4] = True
        assert not E.flags().any()
        st = E.exchange_stats().reshape(NL, 4, 2)
        hs = E.hmc_stats()
    assert npair == NL * (NR // 2 * 2 + NR // 2 * 1) and (st[:, :3, 0] == [NR // 2, NR // 2, NR // 2]).all()
    print("HMC acceptance", hs[:, 1].sum() / hs[:, 0].sum(), flush=True)
    # <phi^2> per rung
    phi2 = (s2 / (NR * V)).reshape(NL, 4)
    mean, err = phi2.mean(axis=0), phi2.std(axis=0, ddof=1) / np.sqrt(NL)
    want = C * C * exact
    print("phi2", mean, "+-", err, "want", want, flush=True)
    assert (err < 0.005 * want).all(), (err, want)
    assert (np.abs(mean - want) <= 5.0 * err).all(), (mean, want, err)
    # acceptance per link against the chi^2 model
    rng = np.random.default_rng(2024)
    beta = np.asarray([xm.coef(_record(0.02, 1.0, 0.0, c))[0] for c in C])
    S = C[None, :] ** 2 * rng.chisquare(V, (400000, 4)) / 2.0
    acc = st[:, :3, 1] / st[:, :3, 0]
    amean, aerr = acc.mean(axis=0), acc.std(axis=0, ddof=1) / np.sqrt(NL)
    model = np.asarray([np.minimum(1.0, np.exp(-(beta[i] - beta[i + 1]) * (S[:, i + 1] - S[:, i]))).mean()
                        for i in range(3)])
    print("acceptance", amean, "+-", aerr, "model", model, flush=True)
    # a ladder's 1000 attempts at p = 0.445: binomial sigma 0.0157, 0.002 over 64 ladders; five times that for the
    # attempts' autocorrelation.  The model's own error at 4e5 samples is 0.0007.
    assert (aerr < 0.01).all() and (np.abs(amean - model) <= 5.0 * aerr).all(), (amean, model, aerr)
    # <exp(-Delta)> = 1 over all attempted pairs
    per = em / (npair / NL)
    imean, ierr = per.mean(), per.std(ddof=1) / np.sqrt(NL)
    print("identity", imean, "+-", ierr, flush=True)
    # Delta has sigma 1.8 here (0.127 x the 14 of S_b - S_a): exp(-Delta) is log-normal with sigma (e^3.2 - 1)^1/2 = 5
    # per sample, 0.011 over the 192,000 pairs; 0.05 allows for the autocorrelation of the attempts
    assert ierr < 0.05 and abs(imean - 1.0) <= 5.0 * ierr, (imean, ierr)
    # every walker has been on every rung of its ladder
    assert visited.all(), np.argwhere(~visited)[:8]
