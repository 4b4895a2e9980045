// Bit-sliced pieces of the arbor skeleton (skeleton.hip), written so that the same text runs in a kernel and, serially, in a plain host
// program (tools/skel_host_check.cpp compares them with a per-pixel loop).
//
// An image is held as bit rows: row y is `wpr` 32-bit words, bit x of word wx is the pixel (y, 32 * wx + x); R = 16 uses the lower
// half of one word per row and leaves the upper half zero.  Pixels outside the image are background: the caller passes zero words
// there.  Neighbours are named as Guo and Hall 1989 do, clockwise from north: P2 N, P3 NE, P4 E, P5 SE, P6 S, P7 SW, P8 W, P9 NW.
// A neighbour plane holds in bit x the neighbour of pixel x; bits of a plane above the image's width may hold anything, every result
// is masked by the centre word, whose bits there are zero.
#pragma once

#if defined(__HIPCC__)
#define SKEL_HD __host__ __device__ inline
#else
#define SKEL_HD inline
#endif

namespace skel {

typedef unsigned int u32;

struct Planes {
    u32 c, p2, p3, p4, p5, p6, p7, p8, p9;
};

SKEL_HD int popc(u32 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// bit j = byte j of the 16 bytes held in four little-endian words is non-zero
SKEL_HD u32 nonzero_bits16(const u32 w[4]) {
    u32 bits = 0;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 4; ++k)
            if ((w[i] >> (8 * k)) & 255u) bits |= 1u << (4 * i + k);
    return bits;
}

// bytes 0 / 1 of the four bits of a nibble, as one little-endian word
SKEL_HD u32 bytes_of_nibble(u32 n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }

// the planes of the word `c` from the 3 x 3 words around it: u* the row above, d* the row below, *l / *r the words left / right
SKEL_HD Planes planes(u32 ul, u32 u, u32 ur, u32 l, u32 c, u32 r, u32 dl, u32 d, u32 dr) {
    Planes p;
    p.c = c;
    p.p2 = u;
    p.p3 = (u >> 1) | (ur << 31);
    p.p4 = (c >> 1) | (r << 31);
    p.p5 = (d >> 1) | (dr << 31);
    p.p6 = d;
    p.p7 = (d << 1) | (dl >> 31);
    p.p8 = (c << 1) | (l >> 31);
    p.p9 = (u << 1) | (ul >> 31);
    return p;
}

// the planes of word (y, wx) of an image of `rows` rows; words outside are zero
SKEL_HD Planes planes_at(const u32* bits, int rows, int wpr, int y, int wx) {
    const bool up = y > 0, down = y + 1 < rows, left = wx > 0, right = wx + 1 < wpr;
    const u32* m = bits + y * wpr + wx;
    return planes(up && left ? m[-wpr - 1] : 0u, up ? m[-wpr] : 0u, up && right ? m[-wpr + 1] : 0u, left ? m[-1] : 0u, m[0],
                  right ? m[1] : 0u, down && left ? m[wpr - 1] : 0u, down ? m[wpr] : 0u, down && right ? m[wpr + 1] : 0u);
}

// of four one-bit planes: exactly one set / at least two set / all four set
struct Sum4 {
    u32 one, two_up, four;
};
SKEL_HD Sum4 sum4(u32 a, u32 b, u32 c, u32 d) {
    const u32 s0 = a ^ b, c0 = a & b, s1 = c ^ d, c1 = c & d;         // two half adders
    Sum4 s;
    s.one = (s0 ^ s1) & ~(c0 | c1);
    s.two_up = c0 | c1 | (s0 & s1);
    s.four = c0 & c1;
    return s;
}

// Guo-Hall A1: the pixels of p.c that sub-iteration `sub` (0 or 1) deletes.
//   C == 1 with C = [!P2 & (P3|P4)] + [!P4 & (P5|P6)] + [!P6 & (P7|P8)] + [!P8 & (P9|P2)]
//   2 <= min(N1, N2) <= 3 with N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8), N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9):
//       both at least 2 and not both 4
//   sub 0: (P2|P3|!P5) & P4 == 0;  sub 1: (P6|P7|!P9) & P8 == 0
SKEL_HD u32 deletable(const Planes& p, int sub) {
    const u32 a = p.p9 | p.p2, b = p.p3 | p.p4, c = p.p5 | p.p6, d = p.p7 | p.p8;
    const Sum4 C = sum4(~p.p2 & b, ~p.p4 & c, ~p.p6 & d, ~p.p8 & a);
    const Sum4 n1 = sum4(a, b, c, d);
    const Sum4 n2 = sum4(p.p2 | p.p3, p.p4 | p.p5, p.p6 | p.p7, p.p8 | p.p9);
    const u32 side = sub == 0 ? (p.p2 | p.p3 | ~p.p5) & p.p4 : (p.p6 | p.p7 | ~p.p9) & p.p8;
    return p.c & C.one & n1.two_up & n2.two_up & ~(n1.four & n2.four) & ~side;
}

// the sum of eight one-bit planes as four planes, least significant first (three layers of half and full adders)
struct Sum8 {
    u32 b0, b1, b2, b3;
};
SKEL_HD Sum8 sum8(const u32 v[8]) {
    // pairs: 2-bit numbers
    u32 lo[4], hi[4];
    for (int i = 0; i < 4; ++i) {
        lo[i] = v[2 * i] ^ v[2 * i + 1];
        hi[i] = v[2 * i] & v[2 * i + 1];
    }
    // two 2-bit numbers -> 3 bits, twice
    u32 q0[2], q1[2], q2[2];
    for (int i = 0; i < 2; ++i) {
        const u32 a0 = lo[2 * i], a1 = hi[2 * i], b0 = lo[2 * i + 1], b1 = hi[2 * i + 1];
        const u32 k0 = a0 & b0;
        q0[i] = a0 ^ b0;
        q1[i] = a1 ^ b1 ^ k0;
        q2[i] = (a1 & b1) | (k0 & (a1 ^ b1));
    }
    // two 3-bit numbers (each at most 4) -> 4 bits
    Sum8 s;
    const u32 k0 = q0[0] & q0[1];
    s.b0 = q0[0] ^ q0[1];
    const u32 x1 = q1[0] ^ q1[1];
    s.b1 = x1 ^ k0;
    const u32 k1 = (q1[0] & q1[1]) | (k0 & x1);
    const u32 x2 = q2[0] ^ q2[1];
    s.b2 = x2 ^ k1;
    s.b3 = (q2[0] & q2[1]) | (k1 & x2);
    return s;
}

// adds the counts of the pixels of p.c to out[0 .. 5] = {pixels, tips, junctions, isolated, orth, diag}.
//   B set neighbours, X the 0 -> 1 steps round the ring P2, P3, ..., P9, P2.  tips: X == 1 and B <= 2; junctions: X >= 3; isolated:
//   B == 0; orth: the pairs with the east and the south neighbour; diag: the pairs with the south-east and the south-west neighbour
//   when neither of the two pixels 4-adjacent to both is set (every pair is counted at its upper pixel).
SKEL_HD void count_word(const Planes& p, int out[6]) {
    if (p.c == 0u) return;
    const u32 ring[8] = {p.p2, p.p3, p.p4, p.p5, p.p6, p.p7, p.p8, p.p9};
    u32 step[8];
    for (int k = 0; k < 8; ++k) step[k] = ~ring[k] & ring[(k + 1) & 7];
    const Sum8 B = sum8(ring), X = sum8(step);
    const u32 x_is_1 = X.b0 & ~(X.b1 | X.b2 | X.b3), x_ge_3 = (X.b0 & X.b1) | X.b2 | X.b3;
    const u32 b_le_2 = ~(B.b3 | B.b2 | (B.b1 & B.b0)), b_is_0 = ~(B.b0 | B.b1 | B.b2 | B.b3);
    out[0] += popc(p.c);
    out[1] += popc(p.c & x_is_1 & b_le_2);
    out[2] += popc(p.c & x_ge_3);
    out[3] += popc(p.c & b_is_0);
    out[4] += popc(p.c & p.p4) + popc(p.c & p.p6);
    out[5] += popc(p.c & p.p5 & ~p.p4 & ~p.p6) + popc(p.c & p.p7 & ~p.p8 & ~p.p6);
}

}  // namespace skel
