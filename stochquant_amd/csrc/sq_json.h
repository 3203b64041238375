// sq_json.h -- the JSON reading of the checkpoint files (sq_io.cpp: the slab's <path>.json; sq_phi4_ens_ckpt_format.cpp:
// the ensemble's).  Host only, no HIP header, nothing but the standard library: the ensemble's format check is also
// built as a stand-alone host program (tests/ckpt_format_check.cpp).
//
// Two layers.  The key scanners (json_int, json_uint, json_dbl, json_dims) find `"key":` in a flat object the
// library itself wrote: the slab checkpoint's reader.  json_parse is a strict parser of RFC 8259 into a small
// tree, for a file that is validated before anything is believed: every byte must belong to the grammar, nothing
// may follow the value, a key may appear once per object.  Strings are taken as their bytes; one that holds an
// escape or a control character is refused (no string of these formats needs either).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

namespace sq {
namespace json {

inline bool read_text(const std::string &path, std::string *j, size_t limit = 1u << 16) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    char buf[512];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, fp)) > 0 && j->size() < limit) j->append(buf, n);
    fclose(fp);
    return true;
}

inline bool json_dims(const std::string &j, long long d[3]) {
    const size_t p = j.find("\"dims\":");
    if (p == std::string::npos) return false;
    const size_t b = j.find('[', p);
    return b != std::string::npos && sscanf(j.c_str() + b + 1, "%lld , %lld , %lld", &d[0], &d[1], &d[2]) == 3;
}

inline long long json_int(const std::string &j, const char *key, bool *found) {
    const std::string k = std::string("\"") + key + "\":";
    const size_t p = j.find(k);
    *found = p != std::string::npos;
    return *found ? strtoll(j.c_str() + p + k.size(), nullptr, 10) : 0;
}

// Unsigned 64-bit fields (seed, step): strtoull, so values >= 2^63 round-trip
// (strtoll would saturate them to LLONG_MAX).
inline unsigned long long json_uint(const std::string &j, const char *key, bool *found) {
    const std::string k = std::string("\"") + key + "\":";
    const size_t p = j.find(k);
    *found = p != std::string::npos;
    return *found ? strtoull(j.c_str() + p + k.size(), nullptr, 10) : 0ull;
}

inline double json_dbl(const std::string &j, const char *key, bool *found) {
    const std::string k = std::string("\"") + key + "\":";
    const size_t p = j.find(k);
    *found = p != std::string::npos;
    return *found ? strtod(j.c_str() + p + k.size(), nullptr) : 0.0;
}

// ---- the strict parser ----
struct Value {
    enum Kind { kNull, kBool, kNumber, kString, kArray, kObject } kind = kNull;
    bool b = false;
    // a number: integral (no fraction, no exponent) or not; an integral one as sign and magnitude, `big` when the
    // magnitude does not fit 64 bits.  -0 is the integer 0.
    bool integral = false, neg = false, big = false;
    unsigned long long mag = 0;
    std::string s;
    std::vector<Value> a;
    std::vector<std::pair<std::string, Value>> o;

    const Value *get(const char *key) const {
        for (const auto &kv : o)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
    // An integer in [0, max]: a number without fraction or exponent.
    bool as_uint(unsigned long long max, unsigned long long *out) const {
        if (kind != kNumber || !integral || big || (neg && mag != 0) || mag > max) return false;
        *out = mag;
        return true;
    }
};

class Parser {
public:
    Parser(const std::string &t, std::string *why) : t_(t), why_(why) {}
    bool document(Value *v) {
        ws();
        if (!value(v, 0)) return false;
        ws();
        if (i_ != t_.size()) return fail("bytes behind the JSON value");
        return true;
    }

private:
    static constexpr int kMaxDepth = 8;
    bool fail(const char *m) {
        *why_ = std::string(m) + " at byte " + std::to_string(i_);
        return false;
    }
    void ws() {
        while (i_ < t_.size() && (t_[i_] == ' ' || t_[i_] == '\t' || t_[i_] == '\n' || t_[i_] == '\r')) ++i_;
    }
    bool lit(const char *w) {
        const size_t n = std::char_traits<char>::length(w);
        if (t_.compare(i_, n, w) != 0) return fail("not a JSON value");
        i_ += n;
        return true;
    }
    bool digits() {
        const size_t b = i_;
        while (i_ < t_.size() && t_[i_] >= '0' && t_[i_] <= '9') ++i_;
        return i_ > b;
    }
    bool number(Value *v) {
        v->kind = Value::kNumber;
        v->integral = true;
        if (i_ < t_.size() && t_[i_] == '-') {
            v->neg = true;
            ++i_;
        }
        const size_t b = i_;
        if (!digits()) return fail("not a JSON number");
        if (t_[b] == '0' && i_ - b > 1) {
            i_ = b + 1;
            return fail("a JSON number has no leading zero");
        }
        for (size_t k = b; k < i_; ++k) {
            const unsigned d = (unsigned)(t_[k] - '0');
            if (v->mag > (~0ull - d) / 10) v->big = true;
            v->mag = v->mag * 10 + d;
        }
        if (i_ < t_.size() && t_[i_] == '.') {
            v->integral = false;
            ++i_;
            if (!digits()) return fail("not a JSON number");
        }
        if (i_ < t_.size() && (t_[i_] == 'e' || t_[i_] == 'E')) {
            v->integral = false;
            ++i_;
            if (i_ < t_.size() && (t_[i_] == '+' || t_[i_] == '-')) ++i_;
            if (!digits()) return fail("not a JSON number");
        }
        return true;
    }
    bool string(std::string *s) {
        ++i_;  // the opening quote
        const size_t b = i_;
        while (i_ < t_.size() && t_[i_] != '"') {
            const unsigned char c = (unsigned char)t_[i_];
            if (c < 0x20 || c == '\\' || c >= 0x80) return fail("a string of this format is plain ASCII without escapes");
            ++i_;
        }
        if (i_ >= t_.size()) return fail("unterminated string");
        s->assign(t_, b, i_ - b);
        ++i_;
        return true;
    }
    bool value(Value *v, int depth) {
        if (depth > kMaxDepth) return fail("nested too deep");
        if (i_ >= t_.size()) return fail("the JSON ends early");
        const char c = t_[i_];
        if (c == '{') {
            v->kind = Value::kObject;
            ++i_;
            ws();
            if (i_ < t_.size() && t_[i_] == '}') return ++i_, true;
            for (;;) {
                ws();
                if (i_ >= t_.size() || t_[i_] != '"') return fail("a key is expected");
                std::string k;
                if (!string(&k)) return false;
                if (v->get(k.c_str())) return fail("a key appears twice");
                ws();
                if (i_ >= t_.size() || t_[i_] != ':') return fail("':' is expected");
                ++i_;
                ws();
                v->o.emplace_back(std::move(k), Value());
                if (!value(&v->o.back().second, depth + 1)) return false;
                ws();
                if (i_ < t_.size() && t_[i_] == ',') {
                    ++i_;
                    continue;
                }
                if (i_ < t_.size() && t_[i_] == '}') return ++i_, true;
                return fail("',' or '}' is expected");
            }
        }
        if (c == '[') {
            v->kind = Value::kArray;
            ++i_;
            ws();
            if (i_ < t_.size() && t_[i_] == ']') return ++i_, true;
            for (;;) {
                ws();
                v->a.emplace_back();
                if (!value(&v->a.back(), depth + 1)) return false;
                ws();
                if (i_ < t_.size() && t_[i_] == ',') {
                    ++i_;
                    continue;
                }
                if (i_ < t_.size() && t_[i_] == ']') return ++i_, true;
                return fail("',' or ']' is expected");
            }
        }
        if (c == '"') {
            v->kind = Value::kString;
            return string(&v->s);
        }
        if (c == 't') {
            v->kind = Value::kBool;
            v->b = true;
            return lit("true");
        }
        if (c == 'f') {
            v->kind = Value::kBool;
            return lit("false");
        }
        if (c == 'n') return lit("null");
        if (c == '-' || (c >= '0' && c <= '9')) return number(v);
        return fail("not a JSON value");
    }
    const std::string &t_;
    std::string *why_;
    size_t i_ = 0;
};

inline bool json_parse(const std::string &text, Value *out, std::string *why) { return Parser(text, why).document(out); }

}  // namespace json
}  // namespace sq
