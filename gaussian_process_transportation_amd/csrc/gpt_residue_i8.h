// Balanced 8-bit residues of the integers of k_var_i8, taken with byte dot products and one fp32 quotient (no fp64, no fix-up), and
// the mixed-radix digits that rebuild an integer from its residues.  Plain C++ apart from the dot-product builtin, which has a
// loop beside it: a g++ program includes the file without HIP (tests/test_var_int8_residue_cpu.py).
//
// A non-negative integer u = sum_i b_i 256^i (bytes b_i) is congruent to t = k + sum_i b_i (256^i mod m) modulo m, k any
// constant folded into the sum: one v_dot4_u32_u8 per four bytes, the coefficients 256^i mod m in [0, m) packed four to a word.
// The signed inputs are biased first, and k takes the bias back:
//   * operand x, an integer-valued double with |x| < 2^51 (the kernel: |x| <= 2^p, p <= 50): the low 52 bits of the double
//     x + 1.5 * 2^52 are the integer x + 2^51 — seven bytes, the top one below 16 — and k = (-2^51) mod m;
//   * accumulator a, an int32 with |a| <= 2^30 (the kernel: |a| <= 128^2 NP <= 2^28): u = a + 2^30, four bytes, k = (-2^30) mod m.
// Either way t <= 6 * 255 * 254 + 15 * 254 + 254 < 2^19.  k also carries the bit pattern of the float 1.5 * 2^23 (0x4B400000): an
// integer below 2^22 added to those bits IS the float 1.5 * 2^23 + t, so the dot product's result is used as a float with no
// conversion, and with tf = that - 1.5 * 2^23
//   fmaf(-rintf(tf * fl(1 / m)), m, 1.5 * 2^23 + t) = 1.5 * 2^23 + r          (every value an integer below 2^24: exact)
// holds the residue r in two's complement in its low mantissa bits: the byte to store is the low byte of the float's bits, with no
// conversion either.  r is the balanced residue as it stands for the 13 odd moduli: t / m is at least 1 / (2 m) > 1.9e-3 away
// from a tie, and the fp32 quotient is off by less than 2^19 / 199 * 2^-23 = 3.2e-4, so rintf picks the nearest integer and
// |r| <= (m - 1) / 2 (checked exhaustively over every reachable t by the test).  Modulus 256: t is the low byte of the
// two's-complement value (both biases are multiples of 256), the same formula leaves r in [-128, 128], congruent to t, and the low
// byte is the balanced residue's.
#pragma once
#include <cstdint>

#include "gpt_plan_i8.h"

#if defined(__HIPCC__)
#define GPT_RES_HD __host__ __device__
#else
#define GPT_RES_HD
#endif

namespace gpt {

constexpr double I8_OPERAND_BIAS = 6755399441055744.0;      // 1.5 * 2^52: x + this holds x + 2^51 in its low 52 bits
constexpr int I8_ACC_BIAS = 1 << 30;
constexpr uint32_t I8_FBIAS_BITS = 0x4B400000u;             // the float 1.5 * 2^23; + t < 2^22: the float 1.5 * 2^23 + t
constexpr float I8_FBIAS = 12582912.0f;

struct I8ResTab {
    float m[I8_NMOD], rm[I8_NMOD];           // modulus, fl(1 / modulus)
    uint32_t op_lo[I8_NMOD];                 // 256^0 .. 256^3 mod m, byte i the coefficient of byte i
    uint32_t op_hi[I8_NMOD];                 // 256^4 .. 256^6 mod m, top byte 0
    uint32_t op_k[I8_NMOD];                  // I8_FBIAS_BITS + (-2^51) mod m
    uint32_t acc_k[I8_NMOD];                 // I8_FBIAS_BITS + (-2^30) mod m   (the accumulator's coefficients are op_lo)
};
constexpr I8ResTab make_i8_res_tab() {
    I8ResTab t{};
    for (int j = 0; j < I8_NMOD; ++j) {
        const int m = I8_MODULI[j];
        t.m[j] = (float)m; t.rm[j] = 1.0f / (float)m;
        uint32_t pw = 1 % m, lo = 0, hi = 0;                 // 256^i mod m
        for (int i = 0; i < 7; ++i) {
            if (i < 4) lo |= pw << (8 * i); else hi |= pw << (8 * (i - 4));
            pw = pw * 256 % m;
        }
        t.op_lo[j] = lo; t.op_hi[j] = hi;
        uint32_t p2 = 1 % m, k30 = 0;                        // 2^i mod m
        for (int i = 0; i < 51; ++i) {
            if (i == 30) k30 = (m - p2) % m;
            p2 = p2 * 2 % m;
        }
        t.acc_k[j] = I8_FBIAS_BITS + k30; t.op_k[j] = I8_FBIAS_BITS + (m - p2) % m;
    }
    return t;
}
static constexpr I8ResTab I8_RES_HOST = make_i8_res_tab();
#if defined(__HIPCC__)
static __constant__ I8ResTab c_i8_res = make_i8_res_tab();   // indexed by a wave-uniform modulus number: scalar loads
#endif
GPT_RES_HD inline const I8ResTab& i8_res_tab() {
#if defined(__HIP_DEVICE_COMPILE__)
    return c_i8_res;
#else
    return I8_RES_HOST;
#endif
}

// acc + sum of the four byte products of a and b
GPT_RES_HD inline uint32_t i8_udot4(const uint32_t a, const uint32_t b, const uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    uint32_t s = acc;
    for (int i = 0; i < 4; ++i) s += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return s;
#endif
}

// bits of the float 1.5 * 2^23 + t, t < 2^19  ->  bits of the float 1.5 * 2^23 + r, r the residue of t modulo m: balanced for an
// odd m, in [-128, 128] for 256 (see above)
GPT_RES_HD inline uint32_t i8_balanced_bits(const uint32_t tbits, const float m, const float rm) {
    float tb;
    __builtin_memcpy(&tb, &tbits, 4);
    const float tf = tb - I8_FBIAS;
    const float rb = __builtin_fmaf(-__builtin_rintf(tf * rm), m, tb);
    uint32_t o;
    __builtin_memcpy(&o, &rb, 4);
    return o;
}
// the residue as an integer, and the byte the planes keep of it (the balanced residue for every modulus, 256 included)
GPT_RES_HD inline int i8_bits_int(const uint32_t rbits) { return (int)(rbits & 0x7FFFFFu) - 0x400000; }
GPT_RES_HD inline int i8_bits_byte(const uint32_t rbits) { return (int)(int8_t)(uint8_t)(rbits & 255u); }
// four residues, element e in byte e
GPT_RES_HD inline uint32_t i8_pack_bits(const uint32_t r0, const uint32_t r1, const uint32_t r2, const uint32_t r3) {
    return (r0 & 255u) | ((r1 & 255u) << 8) | ((r2 & 255u) << 16) | (r3 << 24);
}

// the integer x + 2^51 of an integer-valued x, |x| < 2^51, in two words (hi < 2^20)
GPT_RES_HD inline void i8_operand_split(const double x, uint32_t& lo, uint32_t& hi) {
    const double y = x + I8_OPERAND_BIAS;
    uint64_t b;
    __builtin_memcpy(&b, &y, 8);
    lo = (uint32_t)b; hi = (uint32_t)(b >> 32) & 0xFFFFFu;
}
GPT_RES_HD inline uint32_t i8_operand_bits(const uint32_t lo, const uint32_t hi, const I8ResTab& T, const int j) {
    return i8_balanced_bits(i8_udot4(lo, T.op_lo[j], i8_udot4(hi, T.op_hi[j], T.op_k[j])), T.m[j], T.rm[j]);
}
// residue of an int32 accumulator, |a| <= 2^30
GPT_RES_HD inline uint32_t i8_acc_bits(const int32_t a, const I8ResTab& T, const int j) {
    return i8_balanced_bits(i8_udot4((uint32_t)a + (uint32_t)I8_ACC_BIAS, T.op_lo[j], T.acc_k[j]), T.m[j], T.rm[j]);
}

// ---- reconstruction: Garner's mixed-radix digits -----------------------------------------------------------------------------
// r: the 14 balanced residues of an integer C, |C| < M / 2 (M the product of the moduli).  The digits
//   d_i = ((r_i - sum_{l < i} d_l w[l][i]) inv_i) mod m_i, balanced,      w[l][i] = m_0 .. m_{l-1} mod m_i, inv_i = (m_0 .. m_{i-1})^-1 mod m_i
// are computed with inv_i folded into the weights, wi[l][i] = (w[l][i] inv_i) mod m_i, balanced:
//   v = r_i inv_i - sum_{l < i} d_l wi[l][i],   d_i = v - m_i rint(v / m_i)
// — one reduction per digit, and the same integer: the balanced residue modulo an odd m_i is unique.  |v| <= 128 * 127 + 13 * 128 *
// 127 < 2^18, so every partial sum is an integer that fp32 holds and every fma is exact; v / m stays 1 / (2 m) > 1.9e-3 away from
// a tie and the fp32 quotient is off by less than 2^18 / 199 * 2^-23 = 1.6e-4: rintf picks the nearest integer.  Modulus 0 (256)
// has no digit to compute: d_0 = r_0.
struct I8GarnerTab {
    float m[I8_NMOD], rm[I8_NMOD];       // modulus, its reciprocal
    float inv[I8_NMOD];                  // inv_i, balanced
    float nwi[I8_NMOD][I8_NMOD];         // -wi[l][i] (l < i)
};
constexpr int i8_balanced(int x, int m) { x %= m; if (x < 0) x += m; return x > (m - 1) / 2 ? x - m : x; }
constexpr I8GarnerTab make_i8_garner_tab() {
    I8GarnerTab t{};
    for (int i = 0; i < I8_NMOD; ++i) {
        const int m = I8_MODULI[i];
        t.m[i] = (float)m; t.rm[i] = 1.0f / (float)m;
        int prod = 1, w[I8_NMOD] = {};
        for (int l = 0; l < i; ++l) {
            w[l] = prod;
            prod = prod * I8_MODULI[l] % m;
        }
        int inv = 0;
        for (int x = 1; x < m; ++x) if (prod * x % m == 1) inv = x;
        t.inv[i] = (float)i8_balanced(inv, m);
        for (int l = 0; l < I8_NMOD; ++l) t.nwi[l][i] = l < i ? (float)-i8_balanced(w[l] * inv, m) : 0.0f;
    }
    return t;
}
static constexpr I8GarnerTab I8_GARNER = make_i8_garner_tab();

GPT_RES_HD inline void i8_garner_digits(const float (&r)[I8_NMOD], float (&d)[I8_NMOD]) {
    d[0] = r[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 1; i < I8_NMOD; ++i) {
        float v = r[i] * I8_GARNER.inv[i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int l = 0; l < i; ++l) v = __builtin_fmaf(d[l], I8_GARNER.nwi[l][i], v);
        d[i] = __builtin_fmaf(-__builtin_rintf(v * I8_GARNER.rm[i]), I8_GARNER.m[i], v);
    }
}

}  // namespace gpt
