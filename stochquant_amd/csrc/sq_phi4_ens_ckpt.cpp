// sq_phi4_ens_ckpt.cpp -- the phi^4 ensemble's field digest and its checkpoints (sq_phi4_ensemble_digest, _save,
// _load, _checkpoint_info): the part that touches the handle and the device.  The format itself -- the metadata,
// the section table, the .npy header, the host digest, the validation of a set of files -- is
// sq_phi4_ens_ckpt_format.cpp, which has no HIP call.  A load validates everything there and here before the
// handle is touched; a save reads the handle and changes nothing in it.
#include <exception>
#include <memory>

#include "sq_phi4_ens_ckpt_format.h"
#include "sq_phi4_ens_host.h"

using namespace sq;
using ckpt::Meta;
using ckpt::Section;

namespace {

typedef std::vector<unsigned char> Bytes;

uint64_t to_bits(double d) {
    uint64_t b;
    memcpy(&b, &d, sizeof b);
    return b;
}
double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

// Section `name` of a validated state file (parse_meta has checked dtype, shape and bounds), nullptr when absent.
template <class T>
const T *section(const Meta &m, const Bytes &st, const char *name) {
    const Section *s = m.find(name);
    return s ? reinterpret_cast<const T *>(st.data() + s->offset) : nullptr;
}
template <class T>
T *section(const Meta &m, Bytes &st, const char *name) {
    const Section *s = m.find(name);
    return s ? reinterpret_cast<T *>(st.data() + s->offset) : nullptr;
}

// What a validated set of files can still hold that the library refuses: a replica outside create's parameter
// bound, momenta on a shape without room for them, flow coefficients outside the bound.
bool values_ok(const Meta &m, const Bytes &st, std::string *why) {
    const double cl = from_bits(m.clamp_bits);
    const double *dtau = section<double>(m, st, "dtau"), *m2 = section<double>(m, st, "m2");
    const double *lam = section<double>(m, st, "lambda"), *C = section<double>(m, st, "C");
    for (long long r = 0; r < m.R; ++r)
        if (!ens_params_ok(cl, dtau[r], m2[r], lam[r], C[r])) {
            *why = "the parameters of replica " + std::to_string(r) + " break the bound of sq_phi4_ens_create (finite, "
                   "dtau > 0, clamp^2 finite in fp32, dtau * drift(clamp) < 1e30)";
            return false;
        }
    if (m.M() > 0)
        if (const char *e = ens_momenta_shape_error((int)m.sites(), (int)m.Lz)) {
            *why = std::string("momenta: ") + e;
            return false;
        }
    if (m.F() > 0) {
        const double eps = from_bits(m.feps_bits), fm2 = from_bits(m.fm2_bits), fl = from_bits(m.flam_bits);
        if (std::isinf(fm2) || std::isinf(fl)) {
            *why = "the flow's m2 and lambda must be finite (or NaN: the replica's own)";
            return false;
        }
        for (long long r = 0; r < m.R; ++r)
            if (!ens_params_ok(cl, eps, std::isnan(fm2) ? m2[r] : fm2, std::isnan(fl) ? lam[r] : fl, 0.0)) {
                *why = "flow parameters must be finite with eps > 0 and eps * drift(clamp) < 1e30";
                return false;
            }
    }
    return true;
}

int device_digests(sq_phi4_ens *e, int first, int count, unsigned long long *out) {
    int rc = ens_reserve(e->dig, (size_t)e->R);
    if (rc) return rc;
    SQ_HIP(sq::phi4_ens_digest_launch(e->field.data(), (int)e->sites, first, count, e->dig.data(), e->stream));
    SQ_HIP(hipMemcpyAsync(out, e->dig.data(), sizeof(unsigned long long) * (size_t)count, hipMemcpyDeviceToHost,
                          e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

template <class T>
int read_table(const sq::DevBuf<T> &b, T *to, size_t n) {
    if (!to || n == 0) return SQ_OK;
    SQ_HIP(hipMemcpy(to, b.data(), sizeof(T) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int save(sq_phi4_ens *e, const char *path) {
    DeviceGuard g(e->dev);
    SQ_HIP(hipStreamSynchronize(e->stream));
    const size_t R = (size_t)e->R, nt = (size_t)e->nt;
    Meta m;
    m.Lx = e->Lx;
    m.Ly = e->Ly;
    m.Lz = e->Lz;
    m.R = e->R;
    m.loops = e->p.loops;
    m.adapt = e->p.adapt_dtau ? 1 : 0;
    m.clamp_bits = to_bits(e->p.clamp);
    m.xround = e->xround;
    m.csweep = e->csweep;
    m.nlad = e->nlad;
    m.momenta.assign(e->pn, e->pn + 2 * e->pM);
    m.flev.assign(e->flev, e->flev + e->fF);
    m.feps_bits = to_bits(e->feps);
    m.fm2_bits = to_bits(e->fm2);
    m.flam_bits = to_bits(e->flam);
    m.sections = ckpt::layout(m, e->frecs.data() != nullptr, e->mstat.data() != nullptr, e->hstat.data() != nullptr,
                              &m.state_bytes);
    Bytes st((size_t)m.state_bytes, 0);
    {
        unsigned long long *seed = section<unsigned long long>(m, st, "seed"), *step = section<unsigned long long>(m, st, "step");
        double *dtau = section<double>(m, st, "dtau"), *m2 = section<double>(m, st, "m2");
        double *lam = section<double>(m, st, "lambda"), *C = section<double>(m, st, "C");
        double *fd = section<double>(m, st, "frame_dtau"), *fC = section<double>(m, st, "frame_C");
        float *fT = section<float>(m, st, "frame_T"), *fV = section<float>(m, st, "frame_V");
        int *fi = section<int>(m, st, "frame_init"), *fc = section<int>(m, st, "frame_cnt");
        int *ff = section<int>(m, st, "frame_fired"), *fg = section<int>(m, st, "frame_flag");
        int *fe = section<int>(m, st, "frame_exec");
        for (size_t r = 0; r < R; ++r) {
            const sq_phi4_ens::Rep &o = e->rep[r];
            const sq::Phi4EnsFrameState &f = e->fst[r];
            seed[r] = o.seed;
            step[r] = o.step;
            dtau[r] = o.dtau;
            m2[r] = o.m2;
            lam[r] = o.lambda;
            C[r] = o.C;
            fd[r] = f.dtau;
            fC[r] = f.C;
            fT[r] = f.T;
            fV[r] = f.V;
            fi[r] = f.init;
            fc[r] = f.cnt;
            ff[r] = f.fired;
            fg[r] = f.flag;
            fe[r] = f.exec;
        }
    }
    const size_t M = (size_t)e->pM, F = (size_t)e->fF, L = (size_t)(e->p.loops > 0 ? e->p.loops : 0);
    int rc = read_table(e->flags, section<int>(m, st, "flags"), R);
    if (!rc) rc = read_table(e->frecs, section<float>(m, st, "frame_records"), R * 3 * L);
    if (!rc) rc = read_table(e->cG, section<double>(m, st, "corr_G"), R * nt);
    if (!rc) rc = read_table(e->cS1, section<double>(m, st, "corr_S1"), R);
    if (!rc) rc = read_table(e->cN, section<long long>(m, st, "corr_nmeas"), R);
    if (!rc) rc = read_table(e->pG, section<double>(m, st, "pcorr_G"), R * M * nt);
    if (!rc) rc = read_table(e->pN, section<long long>(m, st, "pcorr_nmeas"), R);
    if (!rc) rc = read_table(e->fG, section<double>(m, st, "flow_G"), R * F * nt);
    if (!rc) rc = read_table(e->fS1, section<double>(m, st, "flow_S1"), R * F);
    if (!rc) rc = read_table(e->fN, section<long long>(m, st, "flow_nmeas"), R * F);
    if (!rc) rc = read_table(e->mstat, section<long long>(m, st, "mala_stats"), R * 3);
    if (!rc) rc = read_table(e->hstat, section<long long>(m, st, "hmc_stats"), R * 4);
    if (!rc) rc = read_table(e->xstat, section<long long>(m, st, "exchange_stats"), R * 2);
    if (!rc) rc = read_table(e->walker, section<int>(m, st, "walkers"), R);
    if (!rc) rc = read_table(e->cstat, section<long long>(m, st, "cluster_stats"), R * 5);
    if (rc) return rc;
    m.state_digest = ckpt::digest(st.data(), st.size());
    const std::unique_ptr<float[]> f(new float[R * e->sites]);  // not zeroed first: the copy fills it
    SQ_HIP(hipMemcpy(f.get(), e->field.data(), sizeof(float) * R * e->sites, hipMemcpyDeviceToHost));
    const size_t row = sizeof(float) * e->sites;
    m.field_digest.resize(R);
    ckpt::digest_rows(reinterpret_cast<const unsigned char *>(f.get()), row, R, m.field_digest.data());
    const std::string pre = ckpt::npy_preamble(m.R, m.Lz, m.Ly, m.Lx);
    m.field_bytes = pre.size() + row * R;
    const std::string json = ckpt::write_meta(m), p(path);
    std::string why;
    // the metadata last: a set whose .json is there is complete, or its sizes and digests give it away
    if (!ckpt::write_file_atomic(p, pre.data(), pre.size(), f.get(), row * R, &why) ||
        !ckpt::write_file_atomic(p + ".state", st.data(), st.size(), nullptr, 0, &why) ||
        !ckpt::write_file_atomic(p + ".json", json.data(), json.size(), nullptr, 0, &why))
        return fail(SQ_E_ARG, "sq_phi4_ensemble_save: " + why);
    return SQ_OK;
}

// A table of the handle from its section: allocated at need, zeros where the file has none (one never allocated
// stays so: it reads as zeros).
template <class T>
int write_table(sq::DevBuf<T> &b, const T *from, size_t n) {
    if (n == 0) return SQ_OK;
    if (!from) {
        if (b.data()) SQ_HIP(hipMemset(b.data(), 0, sizeof(T) * n));
        return SQ_OK;
    }
    int rc = ens_reserve(b, n);
    if (rc) return rc;
    SQ_HIP(hipMemcpy(b.data(), from, sizeof(T) * n, hipMemcpyHostToDevice));
    return SQ_OK;
}

int load(sq_phi4_ens *e, const char *path, int fields_only) {
    Meta m;
    Bytes field, st;
    std::string why;
    if (!ckpt::read_checkpoint(path, true, &m, &field, &st, &why)) return fail(SQ_E_ARG, "sq_phi4_ensemble_load: " + why);
    const auto differs = [&](const char *what, const std::string &file, const std::string &mine) {
        return fail(SQ_E_ARG, std::string("sq_phi4_ensemble_load: the checkpoint's ") + what + " (" + file +
                                  ") does not match this ensemble's (" + mine + ")");
    };
    const auto dims = [](long long x, long long y, long long z) {
        return std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(z);
    };
    if (m.Lx != e->Lx || m.Ly != e->Ly || m.Lz != e->Lz)
        return differs("dims", dims(m.Lx, m.Ly, m.Lz), dims(e->Lx, e->Ly, e->Lz));
    if (m.R != e->R) return differs("R", std::to_string(m.R), std::to_string(e->R));
    if (!fields_only) {
        if (m.loops != e->p.loops) return differs("loops", std::to_string(m.loops), std::to_string(e->p.loops));
        if (m.clamp_bits != to_bits(e->p.clamp))
            return differs("clamp", std::to_string(from_bits(m.clamp_bits)), std::to_string(e->p.clamp));
        if (m.adapt != (e->p.adapt_dtau ? 1 : 0))
            return differs("adapt_dtau", std::to_string(m.adapt), std::to_string(e->p.adapt_dtau ? 1 : 0));
        if (!values_ok(m, st, &why)) return fail(SQ_E_ARG, "sq_phi4_ensemble_load: " + why);
    }
    // ---- nothing below refuses the files: the handle changes from here on ----
    DeviceGuard g(e->dev);
    SQ_HIP(hipStreamSynchronize(e->stream));
    const size_t R = (size_t)e->R, nt = (size_t)e->nt;
    const size_t pre = (size_t)m.field_bytes - sizeof(float) * R * e->sites;
    SQ_HIP(hipMemcpy(e->field.data(), field.data() + pre, sizeof(float) * R * e->sites, hipMemcpyHostToDevice));
    std::vector<unsigned long long> dg(R);
    int rc = device_digests(e, 0, e->R, dg.data());
    if (rc) return rc;
    for (size_t r = 0; r < R; ++r)
        if (dg[r] != m.field_digest[r])
            return fail(SQ_E_HIP, "sq_phi4_ensemble_load: the device copy of replica " + std::to_string(r) +
                                      "'s field differs from the file (digest mismatch after the upload)");
    if (fields_only) return SQ_OK;
    {
        const unsigned long long *seed = section<unsigned long long>(m, st, "seed"), *step = section<unsigned long long>(m, st, "step");
        const double *dtau = section<double>(m, st, "dtau"), *m2 = section<double>(m, st, "m2");
        const double *lam = section<double>(m, st, "lambda"), *C = section<double>(m, st, "C");
        e->rec_dirty = true;  // the device records follow rep[] at the next launch, wherever this call ends
        e->frec_dirty = true;
        for (size_t r = 0; r < R; ++r) e->rep[r] = sq_phi4_ens::Rep{dtau[r], m2[r], lam[r], C[r], seed[r], step[r]};
    }
    // the settings first: they size and zero their accumulators.  The setters' checks have been made above
    // (parse_meta, values_ok), so the parts behind them are applied: only an allocation can still fail
    rc = ens_apply_momenta(e, (int)m.M(), m.momenta.data());
    if (rc) return rc;
    {
        const double fm2 = from_bits(m.fm2_bits), fl = from_bits(m.flam_bits);
        rc = ens_apply_flow(e, from_bits(m.feps_bits), (int)m.F(), m.flev.data(), fm2, fl);
        if (rc) return rc;
        e->feps = from_bits(m.feps_bits);
        e->fm2 = fm2;
        e->flam = fl;
    }
    e->nlad = (int)m.nlad;
    e->xround = m.xround;
    e->csweep = m.csweep;
    {
        const double *fd = section<double>(m, st, "frame_dtau"), *fC = section<double>(m, st, "frame_C");
        const float *fT = section<float>(m, st, "frame_T"), *fV = section<float>(m, st, "frame_V");
        const int *fi = section<int>(m, st, "frame_init"), *fc = section<int>(m, st, "frame_cnt");
        const int *ff = section<int>(m, st, "frame_fired"), *fg = section<int>(m, st, "frame_flag");
        const int *fe = section<int>(m, st, "frame_exec");
        for (size_t r = 0; r < R; ++r) {
            sq::Phi4EnsFrameState f{};
            f.dtau = fd[r];
            f.C = fC[r];
            f.T = fT[r];
            f.V = fV[r];
            f.init = fi[r];
            f.cnt = fc[r];
            f.fired = ff[r];
            f.flag = fg[r];
            f.exec = fe[r];
            e->fst[r] = f;
        }
    }
    const size_t M = (size_t)e->pM, F = (size_t)e->fF, L = (size_t)(e->p.loops > 0 ? e->p.loops : 0);
    rc = write_table(e->flags, section<int>(m, st, "flags"), R);
    // no frames call behind the saver: none behind this handle either (sq_phi4_ens_stability's n)
    if (!m.find("frame_records")) e->frecs = sq::DevBuf<float>();
    if (!rc) rc = write_table(e->frecs, section<float>(m, st, "frame_records"), R * 3 * L);
    if (!rc) rc = write_table(e->cG, section<double>(m, st, "corr_G"), R * nt);
    if (!rc) rc = write_table(e->cS1, section<double>(m, st, "corr_S1"), R);
    if (!rc) rc = write_table(e->cN, section<long long>(m, st, "corr_nmeas"), R);
    if (!rc) rc = write_table(e->pG, section<double>(m, st, "pcorr_G"), R * M * nt);
    if (!rc) rc = write_table(e->pN, section<long long>(m, st, "pcorr_nmeas"), R);
    if (!rc) rc = write_table(e->fG, section<double>(m, st, "flow_G"), R * F * nt);
    if (!rc) rc = write_table(e->fS1, section<double>(m, st, "flow_S1"), R * F);
    if (!rc) rc = write_table(e->fN, section<long long>(m, st, "flow_nmeas"), R * F);
    if (!rc) rc = write_table(e->mstat, section<long long>(m, st, "mala_stats"), R * 3);
    if (!rc) rc = write_table(e->hstat, section<long long>(m, st, "hmc_stats"), R * 4);
    if (!rc) rc = write_table(e->xstat, section<long long>(m, st, "exchange_stats"), R * 2);
    if (!rc) rc = write_table(e->walker, section<int>(m, st, "walkers"), R);
    if (!rc) rc = write_table(e->cstat, section<long long>(m, st, "cluster_stats"), R * 5);
    if (rc) return rc;
    SQ_HIP(hipDeviceSynchronize());  // the memsets ran on the null stream
    e->rec_dirty = true;  // the device records follow rep[] at the next launch
    e->frec_dirty = true;
    e->steps_total = 0;  // perf() restarts
    e->launches = 0;
    return SQ_OK;
}

int info(const char *path, int verify, long long out[8], double *clamp) {
    Meta m;
    Bytes st;
    std::string why;
    if (!ckpt::read_checkpoint(path, verify != 0, &m, nullptr, &st, &why) || (verify && !values_ok(m, st, &why)))
        return fail(SQ_E_ARG, "sq_phi4_ensemble_checkpoint_info: " + why);
    const long long v[8] = {ckpt::kVersion, m.Lx, m.Ly, m.Lz, m.R, m.loops, m.adapt, (long long)m.sections.size()};
    memcpy(out, v, sizeof v);
    if (clamp) *clamp = from_bits(m.clamp_bits);
    return SQ_OK;
}

// No exception crosses the C ABI (std::bad_alloc on a large ensemble, ...).
template <class Body>
int guarded(const char *call, Body body) {
    try {
        return body();
    } catch (const std::exception &x) {
        return fail(SQ_E_ARG, std::string(call) + ": " + x.what());
    } catch (...) {
        return fail(SQ_E_ARG, std::string(call) + ": unexpected exception");
    }
}

}  // namespace

extern "C" {

int sq_phi4_ensemble_digest(sq_phi4_ens *e, int first, int count, unsigned long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    return device_digests(e, first, count, out);
}

int sq_phi4_ensemble_save(sq_phi4_ens *e, const char *path) {
    if (!e || !path) return fail(SQ_E_ARG, "null argument");
    return guarded("sq_phi4_ensemble_save", [&] { return save(e, path); });
}

int sq_phi4_ensemble_load(sq_phi4_ens *e, const char *path, int fields_only) {
    if (!e || !path) return fail(SQ_E_ARG, "null argument");
    return guarded("sq_phi4_ensemble_load", [&] { return load(e, path, fields_only); });
}

int sq_phi4_ensemble_checkpoint_info(const char *path, int verify, long long out[8], double *clamp) {
    if (!path || !out) return fail(SQ_E_ARG, "null argument");
    return guarded("sq_phi4_ensemble_checkpoint_info", [&] { return info(path, verify, out, clamp); });
}

}  // extern "C"
