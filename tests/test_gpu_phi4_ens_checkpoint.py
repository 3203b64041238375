"""Checkpoint, bit-exact resume and the field digest of the phi^4 ensemble on the GPU (sq_phi4_ensemble_save, _load,
_checkpoint_info, _digest).

The digest is compared with the NumPy statement of the header's definition (phi4_ens_checkpoint_format.py), exactly:
it is an integer.  Resume parity, for a script (A, B) of calls: handle X runs A then B; handle Y runs A, saves and is
destroyed; handle Z is created with other seeds, parameters, settings and start field, loads, and runs B.  B's return
values and afterwards every getter must agree between X and Z as bytes -- no tolerance anywhere in this file.  The
refusal tests damage files on the host; the load refuses them before any launch."""
import json
import os

import numpy as np
import pytest

import phi4_ens_checkpoint_format as fmt

pytestmark = pytest.mark.gpu

SHAPE, R, LOOPS = (8, 8, 8), 6, 20
SEEDS = [99, 1234, 0xDEADBEEF12345, 7, 2 ** 63 + 11, 5]
DTAU = [0.19, 0.01, 0.19, 0.01, 0.05, 0.01]  # 0.19 rolls frames back from init_field(0.3); 0.01 climbs by 1 / 0.95


def ens(shape=SHAPE, R=R, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", 0.01)
    kw.setdefault("seeds", SEEDS[:R] if R <= len(SEEDS) else None)
    kw.setdefault("loops", LOOPS)
    E = Phi4Ensemble(shape, R, **kw)
    E.init_field(0.3)
    return E


def other(shape=SHAPE, R=R, **kw):
    """A handle of the same identity and nothing else in common: seeds, parameters, settings, counters, field."""
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("loops", LOOPS)
    Z = Phi4Ensemble(shape, R, dtau=0.02, m2=0.5, lam=0.3, C=0.7, seeds=[1000 + r for r in range(R)], **kw)
    Z.upload(np.ones(Z.lattice_shape, dtype=np.float32))
    Z.set_momenta([(2, 1)])
    Z.set_flow(0.03, levels=(2,), m2=0.25)
    if R % 2 == 0:
        Z.set_ladder(2)
    Z.step(3, every=1, correlate=True, momenta=True)
    Z.step_mala(2)
    Z.exchange_round = 17
    Z.cluster_sweep = 23
    return Z


def state(E):
    s = {"download": E.download(), "params": E.get_params(), "step": E.step_counter, "dtau": E.dtau, "flags": E.flags(),
         "stability": E.stability(), "corr": E.corr_sums(), "momenta": E.momenta, "pcorr": E.pcorr_sums(),
         "flow": E.flow, "mala": E.mala_stats(), "hmc": E.hmc_stats(), "ladder": E.ladder, "xround": E.exchange_round,
         "xstats": E.exchange_stats(), "walkers": E.walkers(), "csweep": E.cluster_sweep, "cstats": E.cluster_stats(),
         "digest": E.digest()}
    if s["flow"]:
        s["fcorr"] = E.fcorr_sums()
    return s


def bits(x):
    """x with every array and float as its bytes: equality is equality of integer views."""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in sorted(x.items())}
    if isinstance(x, (tuple, list)):
        return [bits(v) for v in x]
    if isinstance(x, (float, np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        return (a.dtype.str, a.shape, a.tobytes())
    return x


def differing(a, b):
    return [k for k in a if a[k] != b.get(k)]


def resume(tmp_path, make, A, B, shape=SHAPE, nrep=R, **kw):
    """The method of the module's docstring; returns (path, X's B values, X's final state, Z)."""
    with make() as X:
        A(X)
        want = bits(B(X))
        want_state = bits(state(X))
    path = os.path.join(str(tmp_path), "ck.npy")
    with make() as Y:
        A(Y)
        Y.save(path)
    Z = other(shape, nrep, **kw)
    Z.load(path)
    got = bits(B(Z))
    assert got == want
    got_state = bits(state(Z))
    assert got_state == want_state, differing(want_state, got_state)
    return path, want, want_state, Z


# ---- the digest ----
def awkward_fields(shape, nrep, seed=3):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((nrep, shape[2], shape[1], shape[0])).astype(np.float32)
    flat = phi.reshape(nrep, -1)
    flat[0, :6] = [-0.0, 0.0, np.inf, -np.inf, np.nan, 1.0]
    flat[1, -1] = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]  # another NaN payload, the last site
    flat[1, 0] = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]
    return phi


@pytest.mark.parametrize("shape", [(8, 2, 2), (16, 4, 31), (8, 17, 31), (64, 256, 2)])
def test_digest_is_the_numpy_definition(gpu, shape):
    """32 sites in one wave with most lanes idle; a partial last wave; sites / 4 no multiple of 64; 32,768 sites."""
    from stochquant_amd import Phi4Ensemble
    nrep = 5
    phi = awkward_fields(shape, nrep)
    want = np.array([fmt.field_digest(phi[r]) for r in range(nrep)], dtype=np.uint64)
    assert len(set(want.tolist())) == nrep
    with Phi4Ensemble(shape, nrep, seeds=SEEDS[:nrep]) as E:
        E.upload(phi)
        before = bits({k: v for k, v in state(E).items() if k != "digest"})
        assert np.array_equal(E.digest(), want)
        for first, count in ((0, 1), (1, 3), (4, 1), (2, 0), (0, nrep)):
            assert np.array_equal(E.digest(first, count), want[first:first + count]), (first, count)
        assert E.digest().dtype == np.uint64
        assert bits({k: v for k, v in state(E).items() if k != "digest"}) == before  # it reads and changes nothing
        sites = shape[0] * shape[1] * shape[2]
        for r, site in ((2, 0), (3, sites - 1), (4, sites // 2 + 1)):  # one bit, one replica
            mod = phi.copy()
            w = mod.reshape(nrep, -1).view(np.uint32)
            w[r, site] ^= np.uint32(1 << 13)
            E.upload(mod)
            got = E.digest()
            assert got[r] == fmt.field_digest(mod[r]) and got[r] != want[r]
            assert np.array_equal(np.delete(got, r), np.delete(want, r))
        mod = phi.copy()
        f = mod.reshape(nrep, -1)
        assert f[2, 3] != f[2, sites - 5]
        f[2, [3, sites - 5]] = f[2, [sites - 5, 3]]  # the same values at other sites
        E.upload(mod)
        assert E.digest(2, 1)[0] == fmt.field_digest(mod[2]) != want[2]


# ---- resume parity ----
def params(E):
    E.set_params(dtau=DTAU, m2=[1.0, 0.8, 1.0, 1.2, 1.0, 0.9], lam=[1.0, 1.0, 0.5, 1.0, 2.0, 1.0])


def test_resume_euler_and_heun_steps_with_measurements(gpu, tmp_path):
    def A(E):
        E.set_params(m2=[1.0, 0.8, 1.0, 1.2, 1.0, 0.9])
        E.set_momenta([(1, 0), (0, 1), (3, 2)])
        return E.step(40, every=10, correlate=True, momenta=True)

    def B(E):
        return [E.step(20, every=5, correlate=True, momenta=True, scheme="heun"), E.step(7), E.step(6, every=3)]

    _, _, st, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert Z.momenta == [(1, 0), (0, 1), (3, 2)] and (Z.corr_sums()[2] == 4 + 4).all()
        assert (Z.step_counter == 73).all()


def test_resume_frames_of_both_schemes(gpu, tmp_path):
    seen = {}

    def A(E):
        params(E)
        st, dt = E.run_frames(25)
        seen["st"], seen["dt"] = st, dt
        return st, dt

    def B(E):
        return [E.run_frames(10, scheme="heun", measure=True), E.run_frames(8, correlate=True)]

    _, _, _, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert not seen["st"][:, 0].all() and seen["st"][:, 1].all()  # rolled back; never rolled back
        assert 0.01 / 0.95 in seen["dt"][:, 1]                       # the controller's quotient: a long expansion
        assert Z.stability()["M"].shape == (R, LOOPS)                 # the frame records came with the load


def test_resume_flow_measurements(gpu, tmp_path):
    def A(E):
        params(E)
        E.set_flow(0.01, levels=(1, 3), lam=0.7)
        return E.step_flow(20, every=5, correlate=True)

    def B(E):
        return [E.run_frames_flow(4, correlate=True), E.step_flow(10, every=5, correlate=True, scheme="heun")]

    _, _, _, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert Z.flow == {"eps": 0.01, "levels": (1, 3), "m2": None, "lam": 0.7}
        assert (Z.fcorr_sums()[2] > 4).all()


def test_resume_mala_then_hmc(gpu, tmp_path):
    def A(E):
        E.step(30)
        return E.step_mala(10, every=5, correlate=True)

    def B(E):
        return [E.step_hmc(6, nleap=5, randomize=True, every=2, record=True), E.step_mala(3, record=True)]

    _, _, _, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert (Z.mala_stats()[:, 0] == 13).all() and (Z.hmc_stats()[:, 0] == 6).all()


def test_resume_hmc_with_exchange(gpu, tmp_path):
    def A(E):
        E.set_params(C=[1.0, 1.1, 1.2, 1.0, 1.1, 1.2])
        E.set_ladder(3)
        E.step(20)
        return E.step_hmc_exchange(5, ntraj=2, nleap=3, record=True)

    def B(E):
        return E.step_hmc_exchange(6, ntraj=2, nleap=3, every=1, correlate=True, record=True)

    _, _, _, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert Z.ladder == 3 and Z.exchange_round == 11 and Z.exchange_stats()[:, 0].sum() > 0


@pytest.mark.parametrize("shape", [SHAPE, (64, 11, 29)])
def test_resume_cluster_sweeps_and_sums(gpu, tmp_path, shape):
    """(64, 11, 29): the one-image K = 8 class whose improved sweep parks its labels in a device row that no
    checkpoint holds."""
    nrep = R if shape == SHAPE else 2

    def make():
        return ens(shape, nrep)

    def A(E):
        E.step(20)
        E.step_hmc_cluster(3, ntraj=1, nleap=2)
        return E.cluster_improved(2)

    def B(E):
        return [E.step_hmc_cluster(2, ntraj=2, nleap=2, record=True), E.cluster_improved(2, record=True)]

    _, _, _, Z = resume(tmp_path, make, A, B, shape=shape, nrep=nrep)
    with Z:
        assert Z.cluster_sweep == 9 and (Z.cluster_stats()[:, 0] == 9).all()


# ---- edges ----
def test_large_counters_survive(gpu, tmp_path):
    def A(E):
        E.set_ladder(2)
        E.step(10)
        E.step_counter = 2 ** 40 + 5
        E.exchange_round = 2 ** 40 + 5
        E.cluster_sweep = 2 ** 33 + 1

    def B(E):
        return [E.step_hmc_exchange(3, ntraj=1, nleap=2, record=True), E.cluster(2, record=True)]

    path, _, _, Z = resume(tmp_path, ens, A, B)
    with Z:
        assert (Z.step_counter == 2 ** 40 + 8).all() and Z.exchange_round == 2 ** 40 + 8 and Z.cluster_sweep == 2 ** 33 + 3
    m = fmt.read(path)[0]
    assert m["exchange_round"] == 2 ** 40 + 5 and m["cluster_sweep"] == 2 ** 33 + 1


def test_special_values_survive_bit_for_bit(gpu, tmp_path):
    phi = awkward_fields(SHAPE, R)

    def A(E):
        E.upload(phi[:1], first=0)      # NaN, the infinities, -0.0
        E.step(1)                       # replica 0's guard fires: its flag is set
        E.upload(phi)                   # two NaN payloads
        E.set_stability([np.inf, 1.0, 2.0, 3.0, 4.0, 5.0], [1.0, np.inf, 2.0, 3.0, 4.0, 5.0])

    def B(E):
        return E.run_frames(2)

    path, _, _, Z = resume(tmp_path, ens, A, B)
    Z.close()
    m, fields, st = fmt.read(path)
    assert fields.view(np.uint32).tolist() == phi.view(np.uint32).tolist()
    assert st["flags"][0] != 0 and np.isinf(st["frame_T"][0]) and np.isinf(st["frame_V"][1])


def test_a_fresh_handle_saves_and_loads_zeros(gpu, tmp_path):
    path, _, _, Z = resume(tmp_path, ens, lambda E: None, lambda E: E.step(5, every=5))
    with Z:
        assert not Z.mala_stats().any() and not Z.hmc_stats().any() and Z.momenta == [] and Z.flow is None
        assert Z.stability()["M"].shape == (R, 0) and Z.ladder == 0 and Z.exchange_round == 0
    names = {s["name"] for s in fmt.read(path)[0]["sections"]}
    assert not names & set(fmt.OPTIONAL) and "pcorr_G" not in names and "flow_G" not in names


def test_resume_on_a_shape_without_room_for_momenta(gpu, tmp_path):
    """(8, 2, 2048): a legal shape on which sq_phi4_ens_set_momenta refuses even an empty list.  A load there
    applies "no momenta" without asking the setter, a fresh handle saves and loads, and restore builds it."""
    from stochquant_amd import Phi4Ensemble, StochQuantError
    shape, nrep = (8, 2, 2048), 2
    path = os.path.join(str(tmp_path), "ck.npy")

    def B(E):
        return [E.step(6, every=3, correlate=True), E.run_frames(2)]

    with Phi4Ensemble(shape, nrep, seeds=[5, 6], loops=4) as F:  # a fresh handle
        with pytest.raises(StochQuantError):
            F.set_momenta([])
        F.save(path)
    with Phi4Ensemble(shape, nrep, seeds=[7, 8], loops=4) as Y:
        Y.init_field(0.3)
        Y.step_mala(4)
        Y.load(path)   # back to the fresh state, the MALA counters with it
        assert not Y.mala_stats().any() and not Y.download().any() and (Y.step_counter == 0).all()
        Y.set_params(dtau=[0.01, 0.02], m2=[0.9, 1.1])
        Y.init_field(0.3)
        Y.step(10, every=5, correlate=True)
        Y.save(path)
        want, want_state = bits(B(Y)), bits(state(Y))
    with Phi4Ensemble(shape, nrep, dtau=0.05, C=0.5, seeds=[8, 9], loops=4) as Z:
        Z.step(3)
        Z.load(path)
        assert bits(Z.get_params()["dtau"]) == bits(np.array([0.01, 0.02]))
        assert bits(B(Z)) == want and bits(state(Z)) == want_state
    with Phi4Ensemble.restore(path) as Q:
        assert bits(B(Q)) == want and bits(state(Q)) == want_state


def test_the_saver_continues_as_a_twin_that_did_not_save(gpu, tmp_path):
    def A(E):
        params(E)
        E.set_momenta([(1, 1)])
        E.run_frames(6, correlate=True, momenta=True)
        E.step_mala(4)

    def B(E):
        return [E.run_frames(5), E.step_hmc(3, nleap=2, record=True), E.step(9, every=3, correlate=True, momenta=True)]

    path = os.path.join(str(tmp_path), "ck.npy")
    with ens() as X, ens() as W:
        A(X)
        A(W)
        perf = X.perf()
        X.save(path)
        assert X.perf() == perf
        assert bits(B(X)) == bits(B(W)) and bits(state(X)) == bits(state(W))


def test_two_saves_to_one_path_leave_the_second_and_the_files_are_the_getters(gpu, tmp_path):
    path = os.path.join(str(tmp_path), "ck.npy")
    with ens() as E:
        params(E)
        E.set_momenta([(1, 0), (2, 3)])
        E.set_flow(0.01, levels=(0, 2))
        E.set_ladder(3)
        E.step(10, every=5, correlate=True, momenta=True)
        E.save(path)
        first = E.download()
        E.run_frames(4, correlate=True, flow=True)
        E.step_mala(5)
        E.step_hmc(4, nleap=3)
        E.step_hmc_exchange(3, ntraj=1, nleap=2)
        E.cluster(2)
        E.save(path)
        assert sorted(os.listdir(str(tmp_path))) == ["ck.npy", "ck.npy.json", "ck.npy.state"]
        got = np.load(path)
        assert got.dtype == np.float32 and bits(got) == bits(E.download()) != bits(first)
        m, fields, st = fmt.read(path)  # the NumPy reader: every size, header and digest, and every section
        assert bits(fields) == bits(got) and m["field_digest"] == E.digest().tolist()
        assert m["dims"] == list(SHAPE) and m["R"] == R and m["loops"] == LOOPS and m["adapt_dtau"] == 1
        assert m["clamp_bits"] == fmt.bits(1000.0) and m["ladder"] == 3 and m["exchange_round"] == E.exchange_round
        assert m["cluster_sweep"] == E.cluster_sweep == 2
        assert [tuple(p) for p in m["momenta"]] == E.momenta and tuple(m["flow_levels"]) == E.flow["levels"]
        assert fmt.from_bits(m["flow_eps_bits"]) == 0.01 and np.isnan(fmt.from_bits(m["flow_m2_bits"]))
        assert st["seed"].tolist() == SEEDS
        p, sb = E.get_params(), E.stability()
        G, S1, nm = E.corr_sums()
        pG, pn = E.pcorr_sums()
        fG, fS1, fn = E.fcorr_sums()
        want = {"step": E.step_counter, "dtau": p["dtau"], "m2": p["m2"], "lambda": p["lam"], "C": p["C"],
                "flags": E.flags().astype(np.int32), "frame_dtau": p["dtau"], "frame_C": p["C"],
                "frame_T": sb["T"].astype(np.float32), "frame_V": sb["V"].astype(np.float32), "frame_fired": sb["fired"],
                "frame_records": np.stack([sb["M"], sb["D"], sb["A"]], axis=1), "corr_G": G, "corr_S1": S1,
                "corr_nmeas": nm, "pcorr_G": pG, "pcorr_nmeas": pn, "flow_G": fG, "flow_S1": fS1,
                "mala_stats": E.mala_stats(), "hmc_stats": E.hmc_stats(), "exchange_stats": E.exchange_stats(),
                "walkers": E.walkers(), "cluster_stats": E.cluster_stats()}
        for name, a in want.items():
            assert bits(np.asarray(a).reshape(st[name].shape)) == bits(st[name]), name
        assert (st["flow_nmeas"] == np.asarray(fn)[:, None]).all() and (st["frame_init"] == 1).all()
        assert set(st) == set(want) | {"seed", "flow_nmeas", "frame_init", "frame_cnt", "frame_flag", "frame_exec"}


def test_restore_builds_the_handle(gpu, tmp_path):
    from stochquant_amd import Phi4Ensemble

    def A(E):
        params(E)
        E.set_momenta([(1, 0)])
        E.run_frames(5, correlate=True)

    def B(E):
        return [E.run_frames(3, momenta=True), E.step(4, every=2)]

    def make():
        return ens(clamp=750.0, loops=7, adapt_dtau=False)

    path, want, want_state, Z = resume(tmp_path, make, A, B, clamp=750.0, loops=7, adapt_dtau=False)
    Z.close()
    assert Phi4Ensemble.checkpoint_info(path, verify=True)["clamp"] == 750.0
    with Phi4Ensemble.restore(path) as Q:
        assert Q.shape == SHAPE and Q.R == R and Q.params.loops == 7 and Q.params.clamp == 750.0
        assert bits(B(Q)) == want and bits(state(Q)) == want_state


def test_fields_only_changes_the_fields_and_nothing_else(gpu, tmp_path):
    path = os.path.join(str(tmp_path), "ck.npy")
    with ens(loops=5, clamp=10.0, adapt_dtau=False) as Y:  # only dims and R must match
        Y.set_momenta([(1, 1)])
        Y.step(25, every=5, momenta=True)
        Y.save(path)
        saved, dig = Y.download(), Y.digest()
    with other() as Z:
        Z.run_frames(2)
        before = state(Z)
        Z.load(path, fields_only=True)
        after = state(Z)
        assert bits(after["download"]) == bits(saved) and bits(after["digest"]) == bits(dig)
        for k in ("download", "digest"):
            before.pop(k), after.pop(k)
        assert bits(after) == bits(before), differing(bits(before), bits(after))
        assert Z.stability()["M"].shape == (R, LOOPS)


# ---- refusals ----
def rewrite(path, change):
    with open(path + ".json") as fh:
        m = json.load(fh)
    change(m)
    m["meta_digest"] = fmt.meta_digest(m)
    fmt.write_meta(path, m)


def test_refused_loads_leave_the_handle_as_it_was(gpu, tmp_path):
    from stochquant_amd import StochQuantError

    def A(E):
        params(E)
        E.set_momenta([(1, 0)])
        E.step(12, every=4, correlate=True, momenta=True)

    def B(E):
        return [E.run_frames(3, correlate=True), E.step_mala(4, record=True)]

    with ens() as X:
        A(X)
        want, want_state = bits(B(X)), bits(state(X))
    good = os.path.join(str(tmp_path), "good.npy")
    with ens() as Y:
        Y.step(5)
        Y.set_momenta([(2, 2)])
        Y.save(good)
    with open(good, "rb") as fh:
        field = fh.read()
    with open(good + ".state", "rb") as fh:
        blob = fh.read()
    with open(good + ".json") as fh:
        meta = fh.read()

    def variant(name, f=field, s=blob, change=None):
        p = os.path.join(str(tmp_path), name)
        for suffix, data in (("", f), (".state", s)):
            with open(p + suffix, "wb") as fh:
                fh.write(data)
        with open(p + ".json", "w") as fh:
            fh.write(meta)
        if change:
            rewrite(p, change)
        return p

    def written(name, shape=SHAPE, nrep=R, **kw):
        """A whole checkpoint of another identity, from the NumPy writer."""
        p = os.path.join(str(tmp_path), name)
        args = dict(loops=LOOPS, clamp=1000.0, adapt_dtau=True)
        args.update(kw)
        fmt.write(p, np.zeros((nrep, shape[2], shape[1], shape[0]), dtype=np.float32),
                  fmt.default_state(shape, nrep, args["loops"]), **args)
        return p

    flipped = bytearray(field)
    flipped[len(field) - 9] ^= 0x10
    cases = {"R": (written("R", nrep=R + 1), "R"), "dims": (written("dims", shape=(8, 8, 4)), "dims"),
             "loops": (written("loops", loops=LOOPS + 1), "loops"), "clamp": (written("clamp", clamp=999.0), "clamp"),
             "adapt_dtau": (written("adapt", adapt_dtau=False), "adapt_dtau"),
             "field bit": (variant("bit", f=bytes(flipped)), "digest"),
             "state short": (variant("short", s=blob[:-8]), "state file"),
             "version 2": (variant("v2", change=lambda m: m.update(version=2)), "version 2"),
             "momentum": (variant("mom", change=lambda m: m.update(momenta=[[8, 2]])), "momentum")}
    with ens() as Z:
        A(Z)
        before = bits(state(Z))
        for what, (p, word) in cases.items():
            with pytest.raises(StochQuantError) as ei:
                Z.load(p)
            assert ei.value.code == -1 and word in str(ei.value), (what, str(ei.value))
            if what in ("field bit", "state short", "version 2", "momentum"):  # fields_only reads the same files
                with pytest.raises(StochQuantError):
                    Z.load(p, fields_only=True)
            assert bits(state(Z)) == before, what
        assert bits(B(Z)) == want and bits(state(Z)) == want_state
        Z.load(good)  # and the handle still loads
        assert Z.momenta == [(2, 2)] and (Z.step_counter == 5).all()
