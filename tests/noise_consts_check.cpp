/* CPU check of phi4_noise_consts (stochquant_amd/csrc/sq_noise_consts.h): for
   random (key, step) the fused kernels' evaluation -- a quad's prefix
   {hi(p1), lo(p1), n3}, then rounds 1's xors .. 9 from the launch's noise
   words -- equals the plain ten-round Philox4x32 of sq_rng.h (restated here)
   on the counter {quad, 0, step_lo, step_hi}; step s+1 completed from step
   s's carried prefix equals it too, re-keyed where the two steps differ in
   step_hi (the kernels' noise_rekey, restated). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../stochquant_amd/csrc/sq_noise_consts.h"

using namespace sq;

struct W4 {
    uint32_t x, y, z, w;
};

static W4 philox_plain(W4 c, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += kPhiloxW0;
            k1 += kPhiloxW1;
        }
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c.x, p1 = (uint64_t)kPhiloxM1 * c.z;
        c = W4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    }
    return c;
}

struct Pre {
    uint32_t h1, l1, n3;
};

static Pre prefix(uint32_t quad, uint32_t a0) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * quad;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * ((uint32_t)(p0 >> 32) ^ a0);
    return Pre{(uint32_t)(p1 >> 32), (uint32_t)p1, (uint32_t)p0};
}

static Pre rekey(Pre q, uint32_t da) {
    const uint32_t n2 = q.l1 * kPhiloxM1Inv;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * (n2 ^ da);
    return Pre{(uint32_t)(p1 >> 32), (uint32_t)p1, q.n3};
}

static W4 finish(Pre q, const Phi4NoiseConsts &w, uint32_t k0, uint32_t k1) {
    k0 += 2u * kPhiloxW0;
    k1 += 2u * kPhiloxW1;
    W4 c;
    {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * (q.h1 ^ w.b0), p1 = (uint64_t)kPhiloxM1 * (w.b2 ^ q.n3);
        c = W4{(uint32_t)(p1 >> 32) ^ q.l1 ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ w.d2, (uint32_t)p0};
    }
    for (int r = 3; r < 10; ++r) {
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c.x, p1 = (uint64_t)kPhiloxM1 * c.z;
        c = W4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
    }
    return c;
}

static bool same(W4 a, W4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

static uint64_t s = 0x9E3779B97F4A7C15ull;
static uint64_t nxt(void) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000;
    long bad = 0, checked = 0;
    for (long i = 0; i < n; ++i) {
        const uint32_t k0 = (uint32_t)nxt(), k1 = (uint32_t)nxt();
        uint64_t step = nxt();
        switch (i % 5) {  /* step_lo = 0, 0xFFFFFFFF (step_hi 0 and not), small steps, anything */
        case 0: step &= 0xFFFFFFFF00000000ull; break;
        case 1: step |= 0xFFFFFFFFull; break;
        case 2: step = 0xFFFFFFFFull; break;
        case 3: step &= 0xFFFFull; break;
        default: break;
        }
        const Phi4NoiseConsts w0 = phi4_noise_consts(k0, k1, step), w1 = phi4_noise_consts(k0, k1, step + 1);
        const uint32_t quads[4] = {0u, 0xFFFFFFFFu, (uint32_t)nxt(), (uint32_t)nxt() & 0xFFFFFu};
        for (int j = 0; j < 4; ++j) {
            const uint32_t q = quads[j];
            const W4 r0 = philox_plain(W4{q, 0u, (uint32_t)step, (uint32_t)(step >> 32)}, k0, k1);
            const W4 r1 = philox_plain(W4{q, 0u, (uint32_t)(step + 1), (uint32_t)((step + 1) >> 32)}, k0, k1);
            const Pre p = prefix(q, w0.a0);
            Pre pc = p;  /* step s+1 from the carried prefix */
            if ((w0.a0 ^ w1.a0) != 0u) pc = rekey(pc, w0.a0 ^ w1.a0);
            const bool ok = same(finish(p, w0, k0, k1), r0) && same(finish(pc, w1, k0, k1), r1) &&
                            same(finish(prefix(q, w1.a0), w1, k0, k1), r1);
            if (!ok && bad < 5) printf("k0=%08x k1=%08x step=%016llx quad=%08x\n", k0, k1, (unsigned long long)step, q);
            bad += !ok;
            ++checked;
        }
    }
    printf("checked %ld bad %ld\n", checked, bad);
    return bad != 0;
}
