/* CPU check of sq::Buf (stochquant_amd/csrc/sq_buf.h), the owning buffer behind every buffer of the phi^4
   ensemble's handle, over a malloc-backed policy that counts its calls and can be told to fail the next
   allocation.  Built with the address, leak and undefined-behaviour sanitizers: a double free, a use after a
   free or a block left behind ends the program. */
#include <stdio.h>
#include <stdlib.h>

#include <utility>

#include "../stochquant_amd/csrc/sq_buf.h"

static int g_allocs = 0, g_frees = 0, g_bad = 0;
static bool g_fail_next = false;
static size_t g_last_bytes = 0;

struct CountingAlloc {
    static bool alloc(void **p, size_t bytes) {
        if (g_fail_next) {
            g_fail_next = false;
            return false;
        }
        *p = malloc(bytes);
        if (!*p) return false;
        g_last_bytes = bytes;
        ++g_allocs;
        return true;
    }
    static void free(void *p) {
        ::free(p);
        ++g_frees;
    }
};

typedef sq::Buf<double, CountingAlloc> B;

#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("line %d: %s is false\n", __LINE__, #cond);   \
            ++g_bad;                                             \
        }                                                        \
    } while (0)

static void fill(B &b) {  // every element of the capacity is the buffer's to write
    for (size_t i = 0; i < b.cap(); ++i) b.data()[i] = (double)i;
}

int main() {
    {
        B b;
        CHECK(b.data() == nullptr && b.cap() == 0);
        CHECK(b.reserve(0) && b.data() == nullptr && g_allocs == 0);  // nothing asked, nothing allocated

        /* reserve within the capacity keeps the pointer */
        CHECK(b.reserve(10) && b.data() != nullptr && b.cap() == 10);
        CHECK(g_allocs == 1 && g_last_bytes == 10 * sizeof(double));
        fill(b);
        double *p = b.data();
        CHECK(b.reserve(10) && b.reserve(3) && b.reserve(0));
        CHECK(b.data() == p && b.cap() == 10 && g_allocs == 1 && g_frees == 0);

        /* growth: a new block of the new capacity, the old one freed */
        CHECK(b.reserve(11) && b.cap() == 11 && g_allocs == 2 && g_frees == 1);
        CHECK(g_last_bytes == 11 * sizeof(double));
        fill(b);

        /* a failed growth leaves the buffer empty, and a later reserve succeeds */
        g_fail_next = true;
        CHECK(!b.reserve(100));
        CHECK(b.data() == nullptr && b.cap() == 0 && g_allocs == 2 && g_frees == 2);
        CHECK(b.reserve(5) && b.data() != nullptr && b.cap() == 5 && g_allocs == 3);
        fill(b);

        /* a failed first allocation */
        B c;
        g_fail_next = true;
        CHECK(!c.reserve(4) && c.data() == nullptr && c.cap() == 0 && g_allocs == 3 && g_frees == 2);

        /* move construction leaves the source empty */
        p = b.data();
        B m(std::move(b));
        CHECK(m.data() == p && m.cap() == 5 && b.data() == nullptr && b.cap() == 0);
        CHECK(g_allocs == 3 && g_frees == 2);
        CHECK(b.reserve(2) && b.cap() == 2 && g_allocs == 4);  // the moved-from buffer is an empty one

        /* move assignment frees the overwritten target and leaves the source empty */
        double *q = b.data();
        m = std::move(b);
        CHECK(m.data() == q && m.cap() == 2 && b.data() == nullptr && b.cap() == 0);
        CHECK(g_allocs == 4 && g_frees == 3);
        fill(m);
        B &self = m;
        m = std::move(self);  // onto itself: nothing happens
        CHECK(m.data() == q && m.cap() == 2 && g_frees == 3);
        m = B();  // an empty source: the target is freed
        CHECK(m.data() == nullptr && m.cap() == 0 && g_frees == 4);

        /* three temporaries move-assigned, the all-or-nothing swap of sq_phi4_ens_set_flow */
        B x, y, z, tx, ty, tz;
        CHECK(x.reserve(1) && y.reserve(1) && z.reserve(1));
        g_fail_next = false;
        CHECK(tx.reserve(8) && ty.reserve(8));
        g_fail_next = true;
        const bool ok = tz.reserve(8);
        CHECK(!ok && x.cap() == 1 && y.cap() == 1 && z.cap() == 1);  // the targets are as they were
        CHECK(tz.reserve(8));
        x = std::move(tx);
        y = std::move(ty);
        z = std::move(tz);
        CHECK(x.cap() == 8 && y.cap() == 8 && z.cap() == 8 && tx.cap() == 0 && ty.cap() == 0 && tz.cap() == 0);
        fill(x);
        fill(y);
        fill(z);
        CHECK(g_allocs == 10 && g_frees == 7);
    }
    /* destruction frees what is held, and only that */
    CHECK(g_allocs == 10 && g_frees == 10);
    printf("allocs %d frees %d bad %d\n", g_allocs, g_frees, g_bad);
    return g_bad == 0 && g_allocs == g_frees ? 0 : 1;
}
