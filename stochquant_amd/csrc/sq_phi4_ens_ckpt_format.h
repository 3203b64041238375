// sq_phi4_ens_ckpt_format.h -- the phi^4 ensemble checkpoint's format (include/stochquant.h, "Checkpoints of the
// phi^4 ensemble"): the metadata's reading and writing, the section table of <path>.state, the .npy
// header, the host digest, and the validation of a set of three files.  Pure host C++: no HIP header, no device,
// no handle, nothing of the library but include/stochquant.h's constants.  sq_phi4_ens_ckpt.cpp puts the handle
// and the device behind it; tests/ckpt_format_check.cpp builds it stand-alone under the host sanitizers.
//
// The shape, momentum and flow-level rules live here as well, so that the ensemble's setters
// (sq_phi4_ens_create, sq_phi4_ens_set_momenta, sq_phi4_ens_set_flow) and a load check with the same functions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)
namespace sq {
namespace ckpt {

constexpr const char *kFormatName = "stochquant-phi4-ensemble";
constexpr int kVersion = 1;
constexpr long long kMaxSites = 32768;  // sq::kPhi4EnsMaxSites (sq_phi4_ens.cpp asserts it)

// ---- the ensemble's own rules: nullptr for a legal argument, else what is wrong with it ----
const char *dims_error(long long Lx, long long Ly, long long Lz);
const char *momenta_error(long long Lx, long long Ly, long long M, const int *nxy);
const char *flow_levels_error(long long F, const int *levels);
const char *ladder_error(long long nlad, long long R);

// ---- the digest ----
inline uint64_t mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// sum over i < n of mix(i << 32 | w[i]) mod 2^64, w the little-endian 32-bit words of `bytes`, the last one
// zero-padded where `bytes` is no multiple of 4.
uint64_t digest(const unsigned char *p, size_t bytes);
// out[r] = digest of row r of `rows` rows of row_bytes each, on a few threads where the rows are large.
void digest_rows(const unsigned char *base, size_t row_bytes, size_t rows, uint64_t *out);

// ---- the metadata ----
struct Section {
    std::string name, dtype;       // dtype: "<u8", "<i8", "<f8", "<i4", "<f4"
    std::vector<long long> shape;  // C order
    uint64_t offset = 0;           // in <path>.state, a multiple of 8
    uint64_t bytes() const;
};
struct Meta {
    long long Lx = 0, Ly = 0, Lz = 0, R = 0, loops = 0, adapt = 0;
    uint64_t clamp_bits = 0;
    uint64_t xround = 0, csweep = 0;
    long long nlad = 0;
    std::vector<int> momenta;  // 2 M entries: nx, ny of each
    std::vector<int> flev;     // F levels
    uint64_t feps_bits = 0, fm2_bits = 0, flam_bits = 0;
    std::vector<uint64_t> field_digest;  // R
    uint64_t field_bytes = 0, state_bytes = 0, state_digest = 0;
    std::vector<Section> sections;

    long long sites() const { return Lx * Ly * Lz; }
    long long nt() const { return Lz / 2 + 1; }
    long long M() const { return (long long)momenta.size() / 2; }
    long long F() const { return (long long)flev.size(); }
    const Section *find(const char *name) const;
};

// The sections of a handle of this identity in file order, offsets assigned (each on an 8-byte boundary), and the
// file's size to *bytes.  frame_records, mala, hmc: the optional tables exist.
std::vector<Section> layout(const Meta &m, bool frame_records, bool mala, bool hmc, uint64_t *bytes);

// The digest of the metadata's own values (the key "meta_digest"): `digest` of the little-endian bytes of the
// 64-bit words version, Lx, Ly, Lz, R, loops, clamp_bits, adapt_dtau, exchange_round, cluster_sweep, ladder, M, the
// 2 M momentum numbers, F, the F levels, flow_eps_bits, flow_m2_bits, flow_lambda_bits, field_bytes, state_bytes,
// state_digest, the R field digests, the number of sections and every section's offset in the table's order
// (signed values as two's complement).
uint64_t meta_digest(const Meta &m);
// The whole of <path>.json; no newline behind the closing brace.
std::string write_meta(const Meta &m);
// The .npy preamble (magic, version, header length, header) of a float32 C-order array (R, Lz, Ly, Lx).
std::string npy_preamble(long long R, long long Lz, long long Ly, long long Lx);

// Everything that the metadata alone can show: the JSON complete and strict, format and version, the identity
// legal (dims_error, R >= 1, loops >= 0, adapt_dtau 0 or 1), ladder, momenta and flow levels legal for it, R
// digests, the field file's size that of the shape, and the section table: known names only, every required one
// there once, dtype and shape those of the identity, offsets aligned, inside the file and not overlapping.
bool parse_meta(const std::string &text, Meta *m, std::string *why);

// Whole files, and what ties them to the metadata.
bool read_file(const std::string &path, std::vector<unsigned char> *out, std::string *why);
bool check_field_file(const Meta &m, const std::vector<unsigned char> &file, std::string *why);  // size, header, digests
bool check_state_file(const Meta &m, const std::vector<unsigned char> &file, std::string *why);  // size, digest
// parse_meta of <path>.json, then, verify, the two checks above of <path> and <path>.state (field, state nullable:
// the files' bytes to the caller).
bool read_checkpoint(const std::string &path, bool verify, Meta *m, std::vector<unsigned char> *field,
                     std::vector<unsigned char> *state, std::string *why);

// Temporary-and-rename writing: a, then b, to a new file `path`.tmp.<pid>.<count> beside `path` (count: calls of this
// process, so two threads never share one), flushed to the disk, renamed onto `path`, and the directory flushed;
// the temporary is removed on every failure.  Two saves to one path at one time each leave whole files, but the set
// may be torn between them: a load detects that and refuses it.
bool write_file_atomic(const std::string &path, const void *a, size_t na, const void *b, size_t nb, std::string *why);

}  // namespace ckpt
}  // namespace sq
#pragma GCC visibility pop
