"""The reference of the samplers' interacting-law test (tests/golden/phi4_metropolis.json, written by
tests/golden/make_phi4_metropolis.py), checked without a GPU: the Metropolis sampler reproduces the free
lattice's exact value, a smaller rerun reproduces the fixture, and the fixture has the power the GPU test
(test_gpu_phi4_ens_sampler_edges.py) relies on: the value without the quartic term and the value at C = 1 lie
far from the target, so a sampler of either law would be seen.
"""
import importlib.util
import json
import math
import os

from test_gpu_phi4_ens_heun import _free_phi2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the GPU runs' standard errors, relative to the value: the free-field tests of the same protocols at R = 256 give
# 0.9e-3 (MALA: 0.00016 on 0.1727, test_gpu_phi4_ens_mala.py); at the interacting point the MI355X gave 1.3e-3 for
# MALA and 0.52e-3 for HMC.  The reference has to be three times finer than the finer of the two, and the wrong
# laws far away by the coarser one's measure.
GPU_REL_ERR = {"hmc": 0.52e-3, "mala": 1.3e-3}


def _fixture():
    with open(os.path.join(GOLDEN, "phi4_metropolis.json")) as fh:
        return json.load(fh)


def _generator():
    path = os.path.join(GOLDEN, "make_phi4_metropolis.py")
    spec = importlib.util.spec_from_file_location("make_phi4_metropolis", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixture_is_the_generators():
    ref, gen = _fixture(), _generator()
    assert tuple(ref["shape"]) == gen.SHAPE == (8, 4, 4)
    assert (ref["therm"], ref["seed"], ref["width"]) == (gen.THERM, gen.SEED, gen.WIDTH)
    for name, (par, chains, sweeps) in gen.RUNS.items():
        assert all(ref[name][k] == par[k] for k in ("m2", "lam", "C")), name
        assert (ref[name]["chains"], ref[name]["sweeps"]) == (chains, sweeps), name
    tgt = ref["target"]
    assert (tgt["m2"], tgt["lam"], tgt["C"]) == (0.25, 6.0, 0.7)
    assert (ref["free"]["m2"], ref["free"]["lam"], ref["free"]["C"]) == (0.25, 0.0, 0.7)
    assert (ref["unit_noise"]["m2"], ref["unit_noise"]["lam"], ref["unit_noise"]["C"]) == (0.25, 6.0, 1.0)
    # the reference's error is at most a third of the GPU run's
    assert tgt["sem"] <= min(GPU_REL_ERR.values()) * tgt["phi2"] / 3.0, tgt


def test_the_free_value_is_the_exact_one():
    """lam = 0: <phi^2> = C^2 times the mean over the lattice's modes of 1 / omega, within 4 standard errors,
    for the fixture's long run and for a short one made here."""
    ref, gen = _fixture(), _generator()
    free = ref["free"]
    exact = free["C"] ** 2 * _free_phi2(tuple(ref["shape"]), free["m2"], 0.01)["continuum"]
    assert abs(exact - 0.112917) < 1e-6
    assert abs(free["phi2"] - exact) < 4.0 * free["sem"], (free, exact)
    mean, sem, acc = gen.sample(free["m2"], 0.0, free["C"], 256, 300, 200, 7)
    print(f"METROPOLIS free {mean:.6f} +- {sem:.6f}  exact {exact:.6f}  "
          f"fixture {free['phi2']:.6f} +- {free['sem']:.6f}")
    assert sem < 0.01 * exact and abs(mean - exact) < 4.0 * sem, (mean, sem, exact)
    assert 0.2 < acc < 0.6


def test_a_smaller_run_reproduces_the_fixture():
    ref, gen = _fixture(), _generator()
    tgt = ref["target"]
    mean, sem, _ = gen.sample(tgt["m2"], tgt["lam"], tgt["C"], 256, 300, 100, 11)
    print(f"METROPOLIS target {mean:.6f} +- {sem:.6f}  fixture {tgt['phi2']:.6f} +- {tgt['sem']:.6f}")
    assert sem < 0.005 * tgt["phi2"]
    assert abs(mean - tgt["phi2"]) < 4.0 * math.sqrt(sem * sem + tgt["sem"] ** 2), (mean, sem, tgt)


def test_the_fixture_tells_the_wrong_laws_apart():
    """A sampler without the quartic term, or without the 1 / C^2, would land on the free or the C = 1 value:
    each more than 10 combined standard errors (the coarser GPU run's and the two reference runs') away."""
    ref = _fixture()
    tgt = ref["target"]
    gpu = max(GPU_REL_ERR.values()) * tgt["phi2"]
    for name in ("free", "unit_noise"):
        other = ref[name]
        err = math.sqrt(gpu * gpu + tgt["sem"] ** 2 + other["sem"] ** 2)
        print(f"METROPOLIS {name} {other['phi2']:.6f} is {abs(other['phi2'] - tgt['phi2']) / err:.0f} sigma from "
              f"{tgt['phi2']:.6f}")
        assert abs(other["phi2"] - tgt["phi2"]) > 10.0 * err, (name, other, tgt)
