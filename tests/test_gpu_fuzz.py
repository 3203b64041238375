"""Randomised shape / parameter coverage of the GPU kernels against the oracle
(hypothesis, derandomised so every run checks the same cases).

  * phi^4 step: Lx over every supported row width (one-segment, multi-row and
    multi-segment waves), Ly including partial wave tiles, Lz from 1 (the
    periodic self-neighbour case) upward; C = 0 bit-identical, C = 1 within the
    per-step bound of test_gpu_phi4.py.
  * phi^4 ensemble: legal shapes spread over the four K classes of its
    work-group, two replicas with different parameters; C = 0 and C = 1 (with
    the device's Box-Muller factors) bit-identical, series rows within the
    fsum bound.  The same for its Heun step against the oracle's Heun entry,
    from drawn per-replica start counters up to 2^40.
  * QM1D serial order: random N, loops, Δτ and potID 0 frames with injected
    reference noise, bit-identical frame by frame.
"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from conftest import PHI4_STEP_ATOL, PHI4_STEP_RTOL, tol_report

pytestmark = pytest.mark.gpu

STEP_ATOL = PHI4_STEP_ATOL   # conftest.py: the measured bound (round 6)
STEP_RTOL = PHI4_STEP_RTOL
FUZZ = settings(max_examples=40, deadline=None, derandomize=True,
                suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


@FUZZ
@given(Lx=st.sampled_from([8, 16, 32, 64, 128, 256, 512, 768, 1024]), Ly=st.integers(1, 9),
       Lz=st.integers(1, 12), steps=st.integers(1, 3), C=st.sampled_from([0.0, 1.0]),
       seed=st.integers(0, 2 ** 40), dtau=st.sampled_from([0.005, 0.02, 0.05]))
def test_phi4_random_shapes(gpu, oracle_mod, Lx, Ly, Lz, steps, C, seed, dtau):
    from stochquant_amd import Phi4Lattice
    shape = (Lx, Ly, Lz)
    p = oracle_mod.phi4_params(shape, dtau, 0.5, 1.0, seed, C=C)
    phi = oracle_mod.phi4_init(p, 0.8)
    with Phi4Lattice(shape, dtau=dtau, m2=0.5, lam=1.0, seed=seed, C=C) as L:
        L.upload(phi)
        L.step(steps)
        got = L.download()
    ref = phi
    for s in range(steps):
        ref = oracle_mod.phi4_step(p, ref, s)
    if C == 0.0:
        assert np.array_equal(got, ref)
    else:
        err = np.abs(got.astype(np.float64) - ref)
        tol_report(f"fuzz{shape},dtau={dtau}", err, steps, ref, STEP_RTOL)
        assert np.all(err <= steps * (STEP_ATOL + STEP_RTOL * np.abs(ref)))


# phi^4 ensemble: site counts of the four K classes (K = 1: <= 4,096 sites, 2: <= 8,192, 4: <= 16,384, 8: <= 32,768)
_ENS_BANDS = [(256, 4096), (4097, 8192), (8193, 16384), (16385, 32768)]


@st.composite
def _ens_shapes(draw):
    """Lx, then the target site count of a drawn K class, then a factorisation
    Ly Lz of target // Lx (Lz rounds down: the site count may fall short of
    the target by less than a plane)."""
    Lx = draw(st.sampled_from([8, 16, 32, 64]))
    lo, hi = _ENS_BANDS[draw(st.integers(0, 3))]
    planes = draw(st.integers(lo, hi)) // Lx              # >= 4
    Ly = draw(st.integers(2, planes // 2))
    return (Lx, Ly, planes // Ly)


@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(shape=_ens_shapes(), steps=st.integers(1, 3), every=st.integers(0, 2), C=st.sampled_from([0.0, 1.0]),
       seed=st.integers(0, 2 ** 40), dtau=st.sampled_from([(0.005, 0.02), (0.02, 0.05), (0.05, 0.005)]),
       m2=st.sampled_from([(0.5, -0.5), (1.0, 0.25)]), lam=st.sampled_from([(1.0, 2.0), (4.0, 0.5)]))
def test_phi4_ens_random_shapes(gpu, oracle_mod, bm_tables, shape, steps, every, C, seed, dtau, m2, lam):
    """The ensemble at random legal shapes over all four K, two replicas with
    different Δτ, m², λ and seeds: C = 0 bit for bit the oracle, C = 1 bit for
    bit the oracle with the device's Box-Muller factors; the series rows within
    2 n u Σ|t| of the exactly rounded sums (test_gpu_phi4_ens.py) of the
    oracle's field at that step."""
    import contextlib
    from stochquant_amd import Phi4Ensemble
    from test_gpu_phi4_ens import _exact_sums
    info = Phi4Ensemble.shape_info(shape)                  # raises if the strategy left the legal shapes
    seeds = [seed, seed + 12345]
    ps = [oracle_mod.phi4_params(shape, dtau[r], m2[r], lam[r], seeds[r], C=C) for r in range(2)]
    mode = oracle_mod.device_transcendentals(bm_tables) if C else contextlib.nullcontext()
    with mode:
        ref = [oracle_mod.phi4_init(ps[r], 0.8) for r in range(2)]
        with Phi4Ensemble(shape, 2, dtau=dtau, m2=m2, lam=lam, C=C, seeds=seeds) as E:
            E.upload(np.stack(ref))
            ser = E.step(steps, every=every)
            got = E.download()
        assert (ser is None) if every == 0 else (ser.shape == (steps // every, 2, 4))
        for r in range(2):
            for s in range(steps):
                ref[r] = oracle_mod.phi4_step(ps[r], ref[r], s)
                if every and (s + 1) % every == 0:
                    exact, bound, _ = _exact_sums(ref[r])
                    err = np.abs(ser[(s + 1) // every - 1, r] - exact)
                    assert np.all(err <= bound), (shape, info, r, s, err, bound)
            assert np.array_equal(got[r], ref[r]), (shape, info, r, C, np.max(np.abs(got[r] - ref[r])))


@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(shape=_ens_shapes(), steps=st.integers(1, 3), every=st.integers(0, 2), C=st.sampled_from([0.0, 1.0]),
       seed=st.integers(0, 2 ** 40), dtau=st.sampled_from([(0.005, 0.02), (0.02, 0.05), (0.05, 0.005)]),
       m2=st.sampled_from([(0.5, -0.5), (1.0, 0.25)]), lam=st.sampled_from([(1.0, 2.0), (4.0, 0.5)]),
       step0=st.tuples(st.integers(0, 2 ** 40), st.integers(0, 2 ** 40)).filter(lambda t: t[0] != t[1]))
def test_phi4_ens_heun_random_shapes(gpu, oracle_mod, bm_tables, shape, steps, every, C, seed, dtau, m2, lam, step0):
    """The ensemble's Heun step at random legal shapes over all four K, two
    replicas with different Δτ, m², λ, seeds and start counters (up to 2^40):
    bit for bit the oracle's Heun entry (oracle.phi4_heun_step; at C = 1 with
    the device's Box-Muller factors), the counters advanced by `steps`, no
    guard flag; the series rows within 2 n u Σ|t| of the exactly rounded sums
    of the oracle's field at that step."""
    import contextlib
    from stochquant_amd import Phi4Ensemble
    from test_gpu_phi4_ens import _exact_sums
    info = Phi4Ensemble.shape_info(shape)                  # raises if the strategy left the legal shapes
    seeds = [seed, seed + 12345]
    ps = [oracle_mod.phi4_params(shape, dtau[r], m2[r], lam[r], seeds[r], C=C) for r in range(2)]
    mode = oracle_mod.device_transcendentals(bm_tables) if C else contextlib.nullcontext()
    with mode:
        ref = [oracle_mod.phi4_init(ps[r], 0.8) for r in range(2)]
        with Phi4Ensemble(shape, 2, dtau=dtau, m2=m2, lam=lam, C=C, seeds=seeds) as E:
            E.upload(np.stack(ref))
            E.step_counter = list(step0)
            ser = E.step(steps, every=every, scheme="heun")
            got = E.download()
            assert [int(s) for s in E.step_counter] == [s + steps for s in step0]
            assert not E.flags().any()
        assert (ser is None) if every == 0 else (ser.shape == (steps // every, 2, 4))
        for r in range(2):
            for s in range(steps):
                ref[r], mx = oracle_mod.phi4_heun_step(ps[r], ref[r], step0[r] + s)
                assert max(mx) < ps[r].clampv
                if every and (s + 1) % every == 0:
                    exact, bound, _ = _exact_sums(ref[r])
                    err = np.abs(ser[(s + 1) // every - 1, r] - exact)
                    assert np.all(err <= bound), (shape, info, r, s, err, bound)
            assert np.array_equal(got[r].view(np.uint32), ref[r].view(np.uint32)), \
                (shape, info, r, C, step0, np.max(np.abs(got[r] - ref[r])))


# MALA and HMC: the verdicts the oracle followed, per sampler and K
_sampler_tally = {"mala": {}, "hmc": {}}
_SAMPLER_FUZZ = dict(
    shape=_ens_shapes(), seed=st.integers(0, 2 ** 40),
    step0=st.tuples(st.integers(0, 2 ** 40), st.integers(0, 2 ** 40)).filter(lambda t: t[0] != t[1]),
    m2=st.sampled_from([(0.5, -0.5), (1.0, 0.25)]), lam=st.sampled_from([(1.0, 2.0), (4.0, 0.5)]),
    C=st.tuples(st.sampled_from([0.5, 0.7, 1.0]), st.sampled_from([0.5, 0.7, 1.0])),
    # dtau = 0.4 / sqrt(V) x fac.  With factors of 0.5, 1 and 1.5 nine trajectories in ten are accepted and a K
    # band of some 30 trajectories can go without a rejection (MALA at K = 2: one in two runs on an MI355X, none in a
    # third); with these a CPU run of the same cases rejects 4 of 10 to 17 of 28 per band.
    fac=st.tuples(st.sampled_from([2.0, 3.5, 5.0]), st.sampled_from([2.0, 3.5, 5.0])),
    ntraj=st.integers(1, 4), every=st.integers(0, 2), correlate=st.booleans())


def _sampler_case(o, sampler, shape, seed, step0, m2, lam, C, fac, ntraj, nleap, randomize, every, correlate):
    """Two replicas with different dtau = 0.4 / sqrt(V) x fac, m2, lam, C, seeds and start counters, thermalised
    with 60 Euler steps on the GPU; ntraj trajectories (MALA: nleap = 1) in one call or two; fields, records,
    counters, counts and flags through test_gpu_phi4_ens_hmc.py's check_trajectories; the series rows within
    2 n u sum |t| of the exactly rounded sums of the oracle's field at that point."""
    from stochquant_amd import Phi4Ensemble
    from test_gpu_phi4_ens import _exact_sums
    from test_gpu_phi4_ens_hmc import check_trajectories
    info = Phi4Ensemble.shape_info(shape)                  # raises if the strategy left the legal shapes
    dtau = [0.4 / (shape[0] * shape[1] * shape[2]) ** 0.5 * f for f in fac]
    seeds = [seed, seed + 12345]
    correlate = correlate and every >= 1
    calls = [ntraj] if ntraj == 1 else [ntraj // 2, ntraj - ntraj // 2]
    with Phi4Ensemble(shape, 2, dtau=dtau, m2=m2, lam=lam, C=C, seeds=seeds) as E:
        E.init_field(0.5)
        E.step(60)
        E.step_counter = list(step0)
        start = E.download()
        sers, recs, after = [], [], []
        for n in calls:
            if sampler == "hmc":
                ser, rec = E.step_hmc(n, nleap=nleap, randomize=randomize, every=every, correlate=correlate, record=True)
            else:
                ser, rec = E.step_mala(n, every=every, correlate=correlate, record=True)
                rec = np.concatenate([rec, np.ones((n, 2, 1))], axis=2)      # a trajectory of one step
            assert (ser is None) if every == 0 else (ser.shape == (n // every, 2, 4))
            sers.append(ser)
            recs.append(rec)
            after.append(E.download())
        assert [int(s) for s in E.step_counter] == [s + ntraj for s in step0]
        stats = E.hmc_stats() if sampler == "hmc" else E.mala_stats()
        other = E.mala_stats() if sampler == "hmc" else E.hmc_stats()
        flags, nmeas = E.flags(), E.corr_sums()[2]
    assert not other.any()
    assert list(nmeas) == [sum(n // every for n in calls) if correlate else 0] * 2
    rec = np.concatenate(recs)
    for r in range(2):
        par = (dtau[r], m2[r], lam[r], C[r], seeds[r])
        fields, verdicts, lengths = check_trajectories(o, shape, par, start[r], step0[r], rec[:, r], nleap, randomize)
        done = 0
        for n, ser, got in zip(calls, sers, after):
            for i in range(n // every if every else 0):
                exact, bound, _ = _exact_sums(fields[done + (i + 1) * every - 1])
                err = np.abs(ser[i, r] - exact)
                assert np.all(err <= bound), (shape, info, r, done, i, err, bound)
            done += n
            assert np.array_equal(got[r].view(np.uint32), fields[done - 1].view(np.uint32)), (shape, info, r, done)
        want = [ntraj, verdicts.count(1), verdicts.count(2), sum(lengths)]
        assert list(stats[r]) == (want if sampler == "hmc" else want[:3]), (shape, info, r, stats[r], verdicts, lengths)
        assert bool(flags[r]) == (2 in verdicts), (shape, info, r, verdicts)
        _sampler_tally[sampler].setdefault(info["K"], []).extend(verdicts)


@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(**_SAMPLER_FUZZ)
def test_phi4_ens_mala_random_shapes(gpu, dev_oracle, shape, seed, step0, m2, lam, C, fac, ntraj, every, correlate):
    """The ensemble's MALA step at random legal shapes over all four K (_sampler_case)."""
    _sampler_case(dev_oracle, "mala", shape, seed, step0, m2, lam, C, fac, ntraj, 1, False, every, correlate)


@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(nleap=st.integers(1, 6), randomize=st.booleans(), **_SAMPLER_FUZZ)
def test_phi4_ens_hmc_random_shapes(gpu, dev_oracle, shape, seed, step0, m2, lam, C, fac, ntraj, every, correlate, nleap,
                                    randomize):
    """The ensemble's HMC trajectories at random legal shapes over all four K, nleap = 1 .. 6 fixed or
    randomised (_sampler_case)."""
    _sampler_case(dev_oracle, "hmc", shape, seed, step0, m2, lam, C, fac, ntraj, nleap, randomize, every, correlate)


def test_phi4_ens_sampler_fuzz_saw_both_verdicts(gpu):
    """The two tests above followed accepted and rejected trajectories at every K.  (They run before this one:
    pytest keeps the file's order.)"""
    for sampler, tally in _sampler_tally.items():
        assert set(tally) == {1, 2, 4, 8}, (sampler, sorted(tally))
        for K, vs in sorted(tally.items()):
            print(f"FUZZ {sampler} K = {K}: {len(vs)} trajectories, {vs.count(1)} accepted, {vs.count(0)} rejected, "
                  f"{vs.count(2)} trips", flush=True)
            assert {0, 1} <= set(vs), (sampler, K, vs)


def _exact(res):
    for k in ("stable", "dtau", "lrgEl", "lrgVl", "omega", "runs", "seed"):
        assert res[k][0] == res[k][1], (res["frame"], k, res[k])
    for k in ("f", "x", "xx0"):
        assert np.array_equal(res[k][0], res[k][1]), (res["frame"], k)


@settings(max_examples=25, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(N=st.integers(2, 300), loops=st.integers(1, 30), ratio=st.sampled_from([0.05, 0.3, 2.0, 6.0]),
       a=st.sampled_from([0.05, 0.1, 0.5]), seed=st.integers(1, 2 ** 31 - 1))
def test_serial_order_random_frames(gpu, oracle_mod, N, loops, ratio, a, seed):
    from test_gpu_qm1d_serial import _run_pair
    f0 = 0.3 * np.random.default_rng(seed).standard_normal(N)
    _run_pair(oracle_mod, N, a, ratio * a * a, 0, 1.0, loops, seed, 4, f0, check=_exact)


@settings(max_examples=30, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(Lx=st.sampled_from([16, 64, 256, 512]), Ly=st.integers(1, 6), Lz=st.integers(2, 40),
       nslabs=st.integers(2, 8), ghost=st.integers(1, 8), steps=st.integers(1, 20),
       seed=st.integers(0, 2 ** 40))
def test_slab_decomposition_random(gpu, oracle_mod, monkeypatch, Lx, Ly, Lz, nslabs, ghost, steps, seed):
    """T5 as a property: any slab count and ghost depth gives
    the monolithic field bit for bit, noise on."""
    from stochquant_amd import Phi4Lattice
    nslabs = min(nslabs, Lz)
    shape = (Lx, Ly, Lz)
    p = oracle_mod.phi4_params(shape, 0.02, 0.5, 1.0, seed)
    phi = oracle_mod.phi4_init(p, 0.8)
    with Phi4Lattice(shape, dtau=0.02, m2=0.5, lam=1.0, seed=seed) as L:
        L.upload(phi)
        L.step(steps)
        mono = L.download()
    monkeypatch.setenv("SQ_GHOST", str(ghost))
    with Phi4Lattice(shape, dtau=0.02, m2=0.5, lam=1.0, seed=seed, comm="loopback", nslabs=nslabs) as L:
        L.upload(phi)
        L.step(steps)
        assert np.array_equal(L.download(), mono)
