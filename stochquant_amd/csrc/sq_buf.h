// sq_buf.h -- an owning, move-only buffer of T behind an allocator policy.  Host code only and no HIP header:
// the policies over the HIP allocators live with their user (sq_phi4_ens_host.h), and tests/buf_check.cpp
// instantiates the type over malloc.
//
// Alloc is stateless: static bool alloc(void **p, size_t bytes), static void free(void *p).
#pragma once
#include <cstddef>

namespace sq {

template <class T, class Alloc>
class Buf {
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.forget(); }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_;
            cap_ = o.cap_;
            o.forget();
        }
        return *this;
    }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }

    T *data() const { return p_; }
    size_t cap() const { return cap_; }  // in elements

    // Room for n elements.  Grow-only, and a growth keeps no contents; one that fails leaves the buffer empty.
    bool reserve(size_t n) {
        if (n <= cap_) return true;
        release();
        void *q = nullptr;
        if (!Alloc::alloc(&q, sizeof(T) * n)) return false;
        p_ = static_cast<T *>(q);
        cap_ = n;
        return true;
    }

private:
    void forget() {
        p_ = nullptr;
        cap_ = 0;
    }
    void release() {
        if (p_) Alloc::free(p_);
        forget();
    }
    T *p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace sq
