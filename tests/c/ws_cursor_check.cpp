// Stand-alone check of csrc/workspace.h (host compiler, no HIP, no GPU): a layout measured on a null base bounds the same
// layout carved from any caller's pointer.  Prints "ws cursor ok" and returns 0, or says what failed and returns 1.
#include "workspace.h"

#include <cstdio>
#include <cstdlib>

struct Slices {
    char *a;
    double *b;
    int *c;
    float *d;
    short *e;
    char *end;
};

// a sequence that mixes all four moves, with sizes that are no multiples of 256 (or of anything)
static Slices layout(WsCursor &c) {
    Slices s;
    s.a = c.take<char>(13);
    c.skip(256);
    s.b = c.take256<double>(33);
    s.c = c.take<int>(7);
    c.align256();
    s.d = c.take<float>(65);
    s.e = c.take256<short>(1);
    s.end = c.take<char>(0);
    return s;
}

static int fail(const char *what, unsigned residue) {
    std::printf("ws cursor check failed: %s (base residue %u)\n", what, residue);
    return 1;
}

int main() {
    static_assert(ws_align256(0) == 0 && ws_align256(1) == 256 && ws_align256(256) == 256 && ws_align256(257) == 512, "rounding");
    const unsigned residues[] = {0, 16, 80, 255};
    char *block = static_cast<char *>(std::malloc(8192));
    if (!block) return fail("malloc", 0);
    char *aligned = reinterpret_cast<char *>(ws_align256(reinterpret_cast<uintptr_t>(block)));
    for (int align_base = 0; align_base < 2; ++align_base) {
        WsCursor m(nullptr, align_base != 0);
        const Slices ms = layout(m);
        if (m.bytes() != (align_base ? 256u : 0u) + (size_t)(uintptr_t)ms.end) return fail("bytes() is not allowance + extent", 0);
        for (unsigned r : residues) {
            char *ws = aligned + r;
            WsCursor c(ws, align_base != 0);
            const Slices s = layout(c);
            if (c.bytes() != m.bytes()) return fail("carving and measuring disagree on bytes()", r);
            if (s.a < ws || s.end < ws || (size_t)(s.end - ws) > m.bytes()) return fail("the carve leaves the measured size", r);
            // the slices keep their order and sizes whatever the base
            if ((char *)s.b < s.a + 13 + 256 || (char *)s.c != (char *)(s.b + 33) + (256 - 33 * 8 % 256) ||
                (char *)s.d < (char *)(s.c + 7) || (char *)s.e < (char *)(s.d + 65) || s.end != (char *)s.e + 256)
                return fail("slices overlap or moved", r);
            if (align_base) {
                if ((uintptr_t)s.a != ws_align256((uintptr_t)ws)) return fail("the first slice is not the rounded base", r);
                if ((uintptr_t)s.b % 256 || (uintptr_t)s.e % 256 || (uintptr_t)s.d % 256) return fail("a rounded slice is not 256-byte aligned", r);
            } else if (s.a != ws) {
                return fail("without align_base the first slice is not the caller's pointer", r);
            }
            // every byte of every slice is writable inside the measured size (under -fsanitize=address this is the check)
            for (char *p = s.a; p < s.a + 13; ++p) *p = 1;
            for (int i = 0; i < 33; ++i) reinterpret_cast<char *>(s.b)[8 * i] = 2;
            for (int i = 0; i < 65; ++i) reinterpret_cast<char *>(s.d)[4 * i] = 3;
            if ((size_t)(s.end - ws) > 8192 - 512) return fail("the test block is too small", r);
        }
    }
    std::free(block);
    std::printf("ws cursor ok\n");
    return 0;
}
