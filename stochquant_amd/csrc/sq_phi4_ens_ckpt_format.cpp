// sq_phi4_ens_ckpt_format.cpp -- the phi^4 ensemble checkpoint's format: see sq_phi4_ens_ckpt_format.h.  Pure host
// C++ with no HIP call.
#include "sq_phi4_ens_ckpt_format.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../../include/stochquant.h"
#include "sq_json.h"

namespace sq {
namespace ckpt {

// ---- the ensemble's own rules ----
const char *dims_error(long long Lx, long long Ly, long long Lz) {
    if (Lx != 8 && Lx != 16 && Lx != 32 && Lx != 64) return "a phi^4 ensemble needs Lx in {8, 16, 32, 64}";
    if (Ly < 2 || Lz < 2) return "a phi^4 ensemble needs Ly >= 2 and Lz >= 2";
    if (Ly > kMaxSites || Lz > kMaxSites || Lx * Ly * Lz > kMaxSites)
        return "a phi^4 ensemble needs Lx Ly Lz <= 32768 sites (one LDS image per lattice)";
    return nullptr;
}

const char *momenta_error(long long Lx, long long Ly, long long M, const int *nxy) {
    if (M < 0 || M > SQ_PHI4_ENS_MAX_MOMENTA) return "0 <= M <= SQ_PHI4_ENS_MAX_MOMENTA momenta";
    if (M > 0 && !nxy) return "null argument";
    for (long long m = 0; m < M; ++m)
        if (nxy[2 * m] < 0 || nxy[2 * m] >= Lx || nxy[2 * m + 1] < 0 || nxy[2 * m + 1] >= Ly)
            return "a momentum needs 0 <= nx < Lx and 0 <= ny < Ly";
    return nullptr;
}

const char *flow_levels_error(long long F, const int *levels) {
    if (F < 0 || F > SQ_PHI4_ENS_MAX_FLOW_LEVELS) return "0 <= nlevels <= SQ_PHI4_ENS_MAX_FLOW_LEVELS flow levels";
    if (F > 0 && !levels) return "null argument";
    for (long long l = 0; l < F; ++l)
        if (levels[l] < (l ? levels[l - 1] + 1 : 0) || levels[l] > SQ_PHI4_ENS_MAX_FLOW_STEPS)
            return "flow levels must ascend strictly within [0, SQ_PHI4_ENS_MAX_FLOW_STEPS]";
    return nullptr;
}

const char *ladder_error(long long nlad, long long R) {
    if (nlad != 0 && (nlad < 2 || nlad > R || R % nlad != 0))
        return "nlad must be 0 (no ladders) or lie in [2, nrep] and divide nrep";
    return nullptr;
}

// ---- the digest ----
uint64_t digest(const unsigned char *p, size_t bytes) {
    uint64_t d = 0;
    const size_t whole = bytes / 4;
    for (size_t i = 0; i < whole; ++i) {
        const uint32_t w = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                           ((uint32_t)p[4 * i + 3] << 24);
        d += mix(((uint64_t)i << 32) | w);
    }
    if (bytes % 4) {
        uint32_t w = 0;
        for (size_t k = 0; k < bytes % 4; ++k) w |= (uint32_t)p[4 * whole + k] << (8 * k);
        d += mix(((uint64_t)whole << 32) | w);
    }
    return d;
}

void digest_rows(const unsigned char *base, size_t row_bytes, size_t rows, uint64_t *out) {
    std::atomic<size_t> next{0};
    const auto work = [&] {
        for (size_t r; (r = next.fetch_add(1)) < rows;) out[r] = digest(base + r * row_bytes, row_bytes);
    };
    // a pass over the fields on one core costs as much as writing them: a few threads for anything sizeable
    size_t nt = std::min<size_t>({8, rows, std::max(1u, std::thread::hardware_concurrency())});
    if (rows * row_bytes < (size_t(1) << 20)) nt = 1;
    std::vector<std::thread> th;
    try {
        for (size_t t = 1; t < nt; ++t) th.emplace_back(work);
    } catch (...) {  // no more threads to be had: the ones there, and this one, do the work
    }
    work();
    for (auto &t : th) t.join();
}

// ---- sections ----
namespace {

int dtype_size(const std::string &d) {
    if (d == "<u8" || d == "<i8" || d == "<f8") return 8;
    if (d == "<i4" || d == "<f4") return 4;
    return 0;
}

Section sec(const char *name, const char *dtype, std::vector<long long> shape) {
    Section s;
    s.name = name;
    s.dtype = dtype;
    s.shape = std::move(shape);
    return s;
}

bool optional_section(const std::string &n) { return n == "frame_records" || n == "mala_stats" || n == "hmc_stats"; }

}  // namespace

uint64_t Section::bytes() const {  // all ones where the product does not fit
    uint64_t n = (uint64_t)dtype_size(dtype);
    for (long long s : shape)
        if (s < 0 || __builtin_mul_overflow(n, (uint64_t)s, &n)) return ~0ull;
    return n;
}

uint64_t meta_digest(const Meta &m) {
    std::vector<uint64_t> w = {(uint64_t)kVersion, (uint64_t)m.Lx, (uint64_t)m.Ly, (uint64_t)m.Lz, (uint64_t)m.R,
                               (uint64_t)m.loops, m.clamp_bits, (uint64_t)m.adapt, m.xround, m.csweep, (uint64_t)m.nlad,
                               (uint64_t)m.M()};
    for (int n : m.momenta) w.push_back((uint64_t)(long long)n);
    w.push_back((uint64_t)m.F());
    for (int l : m.flev) w.push_back((uint64_t)(long long)l);
    for (uint64_t x : {m.feps_bits, m.fm2_bits, m.flam_bits, m.field_bytes, m.state_bytes, m.state_digest}) w.push_back(x);
    w.insert(w.end(), m.field_digest.begin(), m.field_digest.end());
    w.push_back((uint64_t)m.sections.size());
    for (const Section &s : m.sections) w.push_back(s.offset);
    std::vector<unsigned char> b(8 * w.size());
    for (size_t i = 0; i < w.size(); ++i)
        for (int k = 0; k < 8; ++k) b[8 * i + (size_t)k] = (unsigned char)(w[i] >> (8 * k));
    return digest(b.data(), b.size());
}

const Section *Meta::find(const char *name) const {
    for (const auto &s : sections)
        if (s.name == name) return &s;
    return nullptr;
}

std::vector<Section> layout(const Meta &m, bool frame_records, bool mala, bool hmc, uint64_t *bytes) {
    const long long R = m.R, nt = m.nt(), M = m.M(), F = m.F();
    std::vector<Section> v;
    for (const char *n : {"seed", "step"}) v.push_back(sec(n, "<u8", {R}));
    for (const char *n : {"dtau", "m2", "lambda", "C"}) v.push_back(sec(n, "<f8", {R}));
    v.push_back(sec("flags", "<i4", {R}));
    for (const char *n : {"frame_dtau", "frame_C"}) v.push_back(sec(n, "<f8", {R}));
    for (const char *n : {"frame_T", "frame_V"}) v.push_back(sec(n, "<f4", {R}));
    for (const char *n : {"frame_init", "frame_cnt", "frame_fired", "frame_flag", "frame_exec"})
        v.push_back(sec(n, "<i4", {R}));
    if (frame_records && m.loops >= 1) v.push_back(sec("frame_records", "<f4", {R, 3, m.loops}));
    v.push_back(sec("corr_G", "<f8", {R, nt}));
    v.push_back(sec("corr_S1", "<f8", {R}));
    v.push_back(sec("corr_nmeas", "<i8", {R}));
    if (M > 0) v.push_back(sec("pcorr_G", "<f8", {R, M, nt}));
    v.push_back(sec("pcorr_nmeas", "<i8", {R}));
    if (F > 0) {
        v.push_back(sec("flow_G", "<f8", {R, F, nt}));
        v.push_back(sec("flow_S1", "<f8", {R, F}));
        v.push_back(sec("flow_nmeas", "<i8", {R, F}));
    }
    if (mala) v.push_back(sec("mala_stats", "<i8", {R, 3}));
    if (hmc) v.push_back(sec("hmc_stats", "<i8", {R, 4}));
    v.push_back(sec("exchange_stats", "<i8", {R, 2}));
    v.push_back(sec("walkers", "<i4", {R}));
    v.push_back(sec("cluster_stats", "<i8", {R, 5}));
    uint64_t at = 0;
    for (auto &s : v) {
        s.offset = at;
        at += (s.bytes() + 7) / 8 * 8;
    }
    if (bytes) *bytes = at;
    return v;
}

// ---- writing ----
namespace {

std::string dec(double v) {
    if (!std::isfinite(v)) return "null";
    char b[40];
    snprintf(b, sizeof b, "%.17g", v);
    return b;
}

double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

template <class T>
std::string list(const std::vector<T> &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

}  // namespace

std::string write_meta(const Meta &m) {
    std::string j = "{\"format\": \"";
    j += kFormatName;
    j += "\", \"version\": " + std::to_string(kVersion);
    j += ",\n \"dims\": " + list(std::vector<long long>{m.Lx, m.Ly, m.Lz});
    j += ", \"R\": " + std::to_string(m.R) + ", \"loops\": " + std::to_string(m.loops);
    j += ", \"clamp_bits\": " + std::to_string(m.clamp_bits) + ", \"clamp\": " + dec(from_bits(m.clamp_bits));
    j += ", \"adapt_dtau\": " + std::to_string(m.adapt);
    j += ",\n \"exchange_round\": " + std::to_string(m.xround) + ", \"cluster_sweep\": " + std::to_string(m.csweep);
    j += ", \"ladder\": " + std::to_string(m.nlad);
    j += ",\n \"momenta\": [";
    for (size_t i = 0; i + 1 < m.momenta.size(); i += 2)
        j += std::string(i ? ", " : "") + "[" + std::to_string(m.momenta[i]) + ", " + std::to_string(m.momenta[i + 1]) + "]";
    j += "], \"flow_levels\": " + list(m.flev);
    j += ",\n \"flow_eps_bits\": " + std::to_string(m.feps_bits) + ", \"flow_eps\": " + dec(from_bits(m.feps_bits));
    j += ", \"flow_m2_bits\": " + std::to_string(m.fm2_bits) + ", \"flow_m2\": " + dec(from_bits(m.fm2_bits));
    j += ", \"flow_lambda_bits\": " + std::to_string(m.flam_bits) + ", \"flow_lambda\": " + dec(from_bits(m.flam_bits));
    j += ",\n \"field_bytes\": " + std::to_string(m.field_bytes) + ", \"state_bytes\": " + std::to_string(m.state_bytes);
    j += ", \"state_digest\": " + std::to_string(m.state_digest);
    j += ", \"meta_digest\": " + std::to_string(meta_digest(m));
    j += ",\n \"field_digest\": " + list(m.field_digest);
    j += ",\n \"sections\": [";
    for (size_t i = 0; i < m.sections.size(); ++i) {
        const Section &s = m.sections[i];
        j += std::string(i ? ",\n  " : "\n  ") + "{\"name\": \"" + s.name + "\", \"dtype\": \"" + s.dtype +
             "\", \"shape\": " + list(s.shape) + ", \"offset\": " + std::to_string(s.offset) + "}";
    }
    j += "]}";
    return j;
}

std::string npy_preamble(long long R, long long Lz, long long Ly, long long Lx) {
    char dict[256];
    snprintf(dict, sizeof dict, "{'descr': '<f4', 'fortran_order': False, 'shape': (%lld, %lld, %lld, %lld), }", R, Lz,
             Ly, Lx);
    std::string hdr(dict);
    const size_t pre = 10;  // magic(6) + version(2) + header length(2)
    hdr.append((64 - (pre + hdr.size() + 1) % 64) % 64, ' ');
    hdr.push_back('\n');
    std::string out("\x93NUMPY\x01", 7);
    out.push_back('\0');
    out.push_back((char)(hdr.size() & 0xFF));
    out.push_back((char)(hdr.size() >> 8));
    return out + hdr;
}

// ---- reading ----
namespace {

using json::Value;

struct Refuse {
    std::string *why;
    bool operator()(const std::string &m) const {
        *why = m;
        return false;
    }
};

// A string of the file inside a message: printable ASCII as it is, '?' for any other byte, 48 bytes at the most.
std::string shown(const std::string &s) {
    std::string o = s.substr(0, 48);
    for (char &c : o)
        if (c < 0x20 || c > 0x7e) c = '?';
    return o;
}

bool as_int(const Value &v, long long lo, long long hi, long long *out) {
    if (v.kind != Value::kNumber || !v.integral || v.big || v.mag > (1ull << 62)) return false;
    const long long x = v.neg ? -(long long)v.mag : (long long)v.mag;
    if (x < lo || x > hi) return false;
    *out = x;
    return true;
}

// An informative decimal copy: a number or null, never read.
bool informative(const Value &v) { return v.kind == Value::kNumber || v.kind == Value::kNull; }

bool int_list(const Value &v, size_t max, long long lo, long long hi, std::vector<long long> *out) {
    if (v.kind != Value::kArray || v.a.size() > max) return false;
    out->clear();
    for (const Value &x : v.a) {
        long long i;
        if (!as_int(x, lo, hi, &i)) return false;
        out->push_back(i);
    }
    return true;
}

}  // namespace

bool parse_meta(const std::string &text, Meta *m, std::string *why) {
    const Refuse no{why};
    Value root;
    std::string perr;
    if (!json::json_parse(text, &root, &perr)) return no("the metadata is not complete JSON: " + perr);
    if (root.kind != Value::kObject) return no("the metadata is not a JSON object");
    static const char *const keys[] = {"format", "version", "dims", "R", "loops", "clamp_bits", "clamp", "adapt_dtau",
                                       "exchange_round", "cluster_sweep", "ladder", "momenta", "flow_levels",
                                       "flow_eps_bits", "flow_eps", "flow_m2_bits", "flow_m2", "flow_lambda_bits",
                                       "flow_lambda", "field_bytes", "state_bytes", "state_digest", "meta_digest",
                                       "field_digest", "sections"};
    for (const auto &kv : root.o)
        if (std::none_of(std::begin(keys), std::end(keys), [&](const char *k) { return kv.first == k; }))
            return no("unknown key \"" + shown(kv.first) + "\" in the metadata");
    for (const char *k : keys)
        if (!root.get(k)) return no(std::string("incomplete metadata: no \"") + k + "\"");
    const Value &fmt = *root.get("format");
    if (fmt.kind != Value::kString || fmt.s != kFormatName)
        return no(std::string("format is not \"") + kFormatName + "\"");
    long long ver;
    if (!as_int(*root.get("version"), 0, 1 << 30, &ver)) return no("version is not an integer");
    if (ver != kVersion) return no("unknown version " + std::to_string(ver) + " (this library reads version 1)");
    *m = Meta();
    std::vector<long long> d;
    if (!int_list(*root.get("dims"), 3, 0, 1 << 30, &d) || d.size() != 3) return no("dims is not a list of three integers");
    m->Lx = d[0];
    m->Ly = d[1];
    m->Lz = d[2];
    if (const char *e = dims_error(m->Lx, m->Ly, m->Lz)) return no(std::string("dims: ") + e);
    if (!as_int(*root.get("R"), 1, 0x7fffffff, &m->R)) return no("R must be an integer >= 1");
    if (!as_int(*root.get("loops"), -0x7fffffffLL - 1, 0x7fffffff, &m->loops)) return no("loops is not a 32-bit integer");
    if (!as_int(*root.get("adapt_dtau"), 0, 1, &m->adapt)) return no("adapt_dtau must be 0 or 1");
    const struct {
        const char *key;
        uint64_t *to;
    } u64s[] = {{"clamp_bits", &m->clamp_bits},     {"exchange_round", &m->xround}, {"cluster_sweep", &m->csweep},
                {"flow_eps_bits", &m->feps_bits},   {"flow_m2_bits", &m->fm2_bits}, {"flow_lambda_bits", &m->flam_bits},
                {"field_bytes", &m->field_bytes},   {"state_bytes", &m->state_bytes},
                {"state_digest", &m->state_digest}};
    for (const auto &u : u64s) {
        unsigned long long x;
        if (!root.get(u.key)->as_uint(~0ull, &x)) return no(std::string(u.key) + " is not an unsigned 64-bit integer");
        *u.to = x;
    }
    for (const char *k : {"clamp", "flow_eps", "flow_m2", "flow_lambda"})
        if (!informative(*root.get(k))) return no(std::string(k) + " is neither a number nor null");
    if (!as_int(*root.get("ladder"), 0, 0x7fffffff, &m->nlad)) return no("ladder is not an integer >= 0");
    if (const char *e = ladder_error(m->nlad, m->R)) return no(std::string("ladder: ") + e);
    const Value &mom = *root.get("momenta");
    if (mom.kind != Value::kArray || mom.a.size() > SQ_PHI4_ENS_MAX_MOMENTA)
        return no("momenta is not a list of at most SQ_PHI4_ENS_MAX_MOMENTA pairs");
    for (const Value &p : mom.a) {
        if (!int_list(p, 2, -0x7fffffff, 0x7fffffff, &d) || d.size() != 2) return no("a momentum is not a pair of integers");
        m->momenta.push_back((int)d[0]);
        m->momenta.push_back((int)d[1]);
    }
    if (const char *e = momenta_error(m->Lx, m->Ly, m->M(), m->momenta.data())) return no(std::string("momenta: ") + e);
    if (!int_list(*root.get("flow_levels"), SQ_PHI4_ENS_MAX_FLOW_LEVELS, -0x7fffffff, 0x7fffffff, &d))
        return no("flow_levels is not a list of at most SQ_PHI4_ENS_MAX_FLOW_LEVELS integers");
    for (long long l : d) m->flev.push_back((int)l);
    if (const char *e = flow_levels_error(m->F(), m->flev.data())) return no(std::string("flow_levels: ") + e);
    const Value &fd = *root.get("field_digest");
    if (fd.kind != Value::kArray || (long long)fd.a.size() != m->R) return no("field_digest is not a list of R digests");
    for (const Value &x : fd.a) {
        unsigned long long u;
        if (!x.as_uint(~0ull, &u)) return no("a field digest is not an unsigned 64-bit integer");
        m->field_digest.push_back(u);
    }
    const uint64_t want = npy_preamble(m->R, m->Lz, m->Ly, m->Lx).size() + 4ull * (uint64_t)m->R * (uint64_t)m->sites();
    if (m->field_bytes != want)
        return no("field_bytes " + std::to_string(m->field_bytes) + " is not the size of a float32 (R, Lz, Ly, Lx) .npy (" +
                  std::to_string(want) + ")");
    // the section table, against every section a handle of this identity can have
    const std::vector<Section> all = layout(*m, true, true, true, nullptr);
    const Value &secs = *root.get("sections");
    if (secs.kind != Value::kArray || secs.a.size() > all.size()) return no("sections is not a list of the known sections");
    for (const Value &sv : secs.a) {
        if (sv.kind != Value::kObject || sv.o.size() != 4 || !sv.get("name") || !sv.get("dtype") || !sv.get("shape") ||
            !sv.get("offset"))
            return no("a section is not {name, dtype, shape, offset}");
        const Value &nm = *sv.get("name"), &dt = *sv.get("dtype");
        if (nm.kind != Value::kString || dt.kind != Value::kString) return no("a section's name and dtype are strings");
        const auto it = std::find_if(all.begin(), all.end(), [&](const Section &s) { return s.name == nm.s; });
        if (it == all.end()) return no("unknown section \"" + shown(nm.s) + "\"");
        if (m->find(nm.s.c_str())) return no("section \"" + nm.s + "\" appears twice");
        Section s;
        s.name = nm.s;
        s.dtype = dt.s;
        if (s.dtype != it->dtype) return no("section \"" + s.name + "\" has dtype " + shown(s.dtype) + ", not " + it->dtype);
        if (!int_list(*sv.get("shape"), 4, 0, 0x7fffffff, &s.shape) || s.shape != it->shape)
            return no("section \"" + s.name + "\" has a shape that disagrees with R, Lz, loops, the momenta or the "
                      "flow levels");
        unsigned long long off;
        if (!sv.get("offset")->as_uint(~0ull, &off) || off % 8 != 0)
            return no("section \"" + s.name + "\" has no offset on an 8-byte boundary");
        s.offset = off;
        if (s.offset > m->state_bytes || s.bytes() > m->state_bytes - s.offset)
            return no("section \"" + s.name + "\" reaches past the end of the state file");
        m->sections.push_back(std::move(s));
    }
    for (const Section &s : all)
        if (!optional_section(s.name) && !m->find(s.name.c_str())) return no("required section \"" + s.name + "\" is missing");
    std::vector<const Section *> by;
    for (const Section &s : m->sections) by.push_back(&s);
    std::sort(by.begin(), by.end(), [](const Section *a, const Section *b) { return a->offset < b->offset; });
    for (size_t i = 1; i < by.size(); ++i)
        if (by[i - 1]->offset + by[i - 1]->bytes() > by[i]->offset)
            return no("sections \"" + by[i - 1]->name + "\" and \"" + by[i]->name + "\" overlap");
    unsigned long long md;
    if (!root.get("meta_digest")->as_uint(~0ull, &md)) return no("meta_digest is not an unsigned 64-bit integer");
    if (md != meta_digest(*m)) return no("the metadata does not have the digest it records (meta_digest)");
    return true;
}

bool read_file(const std::string &path, std::vector<unsigned char> *out, std::string *why) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) {
        *why = "cannot read " + path;
        return false;
    }
    out->clear();
    bool ok = fseek(fp, 0, SEEK_END) == 0;
    const long n = ok ? ftell(fp) : -1;
    ok = ok && n >= 0 && fseek(fp, 0, SEEK_SET) == 0;
    if (ok) {
        out->resize((size_t)n);
        ok = n == 0 || fread(out->data(), 1, (size_t)n, fp) == (size_t)n;
    }
    fclose(fp);
    if (!ok) *why = "cannot read " + path;
    return ok;
}

static std::string shown_header(const std::string &h) {
    std::string o = h.substr(0, std::min<size_t>(h.find_last_not_of(" \n") + 1, 120));
    for (char &c : o)
        if (c < 0x20 || c > 0x7e) c = '?';
    return o;
}

bool check_field_file(const Meta &m, const std::vector<unsigned char> &f, std::string *why) {
    const Refuse no{why};
    const std::string pre = npy_preamble(m.R, m.Lz, m.Ly, m.Lx);
    if (f.size() < 10 || memcmp(f.data(), pre.data(), 8) != 0) return no("the field file is not a NumPy .npy v1.0 file");
    const size_t hl = f[8] | ((size_t)f[9] << 8);
    if (f.size() < 10 + hl) return no("the field file's .npy header is truncated");
    const std::string hdr(reinterpret_cast<const char *>(f.data()) + 10, hl);
    if (hdr != pre.substr(10)) {
        if (hdr.find("'descr': '<f4'") == std::string::npos) return no("the field file's .npy dtype is not '<f4'");
        if (hdr.find("'fortran_order': False") == std::string::npos) return no("the field file's .npy is in Fortran order");
        return no("the field file's .npy header is not that of shape (" + std::to_string(m.R) + ", " +
                  std::to_string(m.Lz) + ", " + std::to_string(m.Ly) + ", " + std::to_string(m.Lx) + "): " +
                  shown_header(hdr));
    }
    if (f.size() != m.field_bytes)
        return no("the field file has " + std::to_string(f.size()) + " bytes, the metadata says " +
                  std::to_string(m.field_bytes));
    const size_t row = 4 * (size_t)m.sites();
    std::vector<uint64_t> got((size_t)m.R);
    digest_rows(f.data() + pre.size(), row, (size_t)m.R, got.data());
    for (long long r = 0; r < m.R; ++r)
        if (got[(size_t)r] != m.field_digest[(size_t)r])
            return no("the field of replica " + std::to_string(r) + " does not have the digest the metadata records");
    return true;
}

bool check_state_file(const Meta &m, const std::vector<unsigned char> &f, std::string *why) {
    const Refuse no{why};
    if (f.size() != m.state_bytes)
        return no("the state file has " + std::to_string(f.size()) + " bytes, the metadata says " +
                  std::to_string(m.state_bytes));
    if (digest(f.data(), f.size()) != m.state_digest) return no("the state file does not have the digest the metadata records");
    return true;
}

bool read_checkpoint(const std::string &path, bool verify, Meta *m, std::vector<unsigned char> *field,
                     std::vector<unsigned char> *state, std::string *why) {
    std::vector<unsigned char> j;
    if (!read_file(path + ".json", &j, why)) return false;
    if (!parse_meta(std::string(j.begin(), j.end()), m, why)) {
        *why = path + ".json: " + *why;
        return false;
    }
    if (!verify) return true;
    std::vector<unsigned char> f, s;
    if (!read_file(path + ".state", &s, why) || !check_state_file(*m, s, why)) return false;
    if (!read_file(path, &f, why) || !check_field_file(*m, f, why)) return false;
    if (field) *field = std::move(f);
    if (state) *state = std::move(s);
    return true;
}

bool write_file_atomic(const std::string &path, const void *a, size_t na, const void *b, size_t nb, std::string *why) {
    // one temporary per call: the process, and a count that two threads of it never share
    static std::atomic<unsigned long long> calls{0};
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid()) + "." + std::to_string(calls.fetch_add(1));
    FILE *fp = fopen(tmp.c_str(), "wbx");  // never onto a file that is there
    if (!fp) {
        *why = "cannot write " + tmp;
        return false;
    }
    bool ok = (na == 0 || fwrite(a, 1, na, fp) == na) && (nb == 0 || fwrite(b, 1, nb, fp) == nb);
    ok = ok && fflush(fp) == 0 && fsync(fileno(fp)) == 0;
    ok = (fclose(fp) == 0) && ok;
    ok = ok && rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) {
        remove(tmp.c_str());
        *why = "cannot write " + path;
        return false;
    }
    // the new name itself reaches the disk with its directory
    const size_t slash = path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : path.substr(0, slash));
    const int fd = open(dir.c_str(), O_RDONLY | O_DIRECTORY);
    if (fd >= 0) {
        (void)fsync(fd);  // a file system that cannot flush a directory has nothing to flush
        close(fd);
    }
    return true;
}

}  // namespace ckpt
}  // namespace sq
