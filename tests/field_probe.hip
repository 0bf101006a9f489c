// field_probe.hip -- applies one primitive of csrc/babybear.hpp / csrc/poseidon2.hpp at a time to arrays of operands and writes the RAW
// result words, so that a test can check the range contract of the lazy and signed forms as well as the congruence.
//
// One source, two programs:
//   hipcc --offload-arch=gfx950 field_probe.hip   -> every operation runs in a kernel (the device forms, inline assembly included)
//   g++ -x c++ field_probe.hip                    -> the same operations run on the host (the host forms)
// usage: field_probe <operand file> <result file>.  Files are little-endian u32 words:
//   in : MAGIC, n_jobs, then per job   0, op, n, n * arity(op) operand words                                  (apply)
//                                  or  1, fast_op, plain_op, start_lo, start_hi, count_lo, count_hi, stride, bias  (exhaustive)
//   out: MAGIC, n_jobs, then per job   n * outw(op) result words                                              (apply)
//                                  or  mismatches_lo, mismatches_hi, first_index_lo, first_index_hi           (exhaustive)
// An exhaustive job compares two unary operations on the operand word (u32)(index - bias) for index = start + k * stride, k < count.
// The "plain" operations (ids >= 100) are uint64_t / int64_t `%` forms written here; tests/field_probe_ref.py checks them against
// Python integers on sampled operands, so the exhaustive passes rest on that reference and not on the headers.
// Every size is checked against the file before anything runs; operands are the caller's business (the tests feed each operation
// only operands inside its stated precondition).
#define ZK_NO_HOST_AVX512 1
#include "babybear.hpp"
#include "poseidon2.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <vector>

#if defined(__HIPCC__)
#define PROBE_HD __host__ __device__
#else
#define PROBE_HD
#endif

using namespace zk;

enum Op : uint32_t {
    OP_RED_2P = 1, OP_MMUL_LAZY, OP_MMUL, OP_MADD, OP_MSUB, OP_MNEG, OP_SMML, OP_CANON_SIGNED, OP_CENTER_SIGNED, OP_SMRED64,
    OP_CANON_SIGNED_WIDE, OP_MRED64, OP_LAZYACC, OP_TO_MONTY, OP_FROM_MONTY, OP_MPOW, OP_MINV, OP_EXT_ADD, OP_EXT_SUB, OP_EXT_MUL,
    OP_EXT_MUL_BASE, OP_EXT_FROBENIUS, OP_EXT_INV, OP_MDOUBLE, OP_MHALVE, OP_MDIV2, OP_MDIV3, OP_MDIV4, OP_MDIV8, OP_MDIV27,
    OP_SBOX7, OP_SBOX7_RCS, OP_SBOX7_RC, OP_P2_EXTERNAL, OP_P2_INTERNAL, OP_P2_PERMUTE, OP_EXT_NEG, OP_EXT_SQR, OP_EXT_POW,
    OP_TWO_ADIC_GEN, OP_BITREV32, OP_P2_COMPRESS, OP_P2_HASH_SLICE, OP_MONTY_ROUNDTRIP, OP_LAST_,
    PL_RED_2P = 100, PL_CANON_SIGNED, PL_CENTER_SIGNED, PL_MHALVE, PL_MDOUBLE, PL_MDIV2, PL_MDIV3, PL_MDIV4, PL_MDIV8, PL_MDIV27,
    PL_SBOX7, PL_IDENTITY, PL_LAST_
};
constexpr uint32_t HASH_SLICE_MAX = 24;   // OP_P2_HASH_SLICE: len, then 24 words of which the first len are absorbed
constexpr uint32_t LAZYACC_MAX_REPS = 1u << 21;
constexpr uint32_t MAX_ITEMS = 1u << 22;

static bool op_shape(uint32_t op, uint32_t* arity, uint32_t* outw) {
    uint32_t a = 0, o = 1;
    switch (op) {
    case OP_RED_2P: case OP_MNEG: case OP_CANON_SIGNED: case OP_CENTER_SIGNED: case OP_CANON_SIGNED_WIDE: case OP_TO_MONTY:
    case OP_FROM_MONTY: case OP_MINV: case OP_MDOUBLE: case OP_MHALVE: case OP_MDIV2: case OP_MDIV3: case OP_MDIV4: case OP_MDIV8:
    case OP_MDIV27: case OP_SBOX7: case OP_TWO_ADIC_GEN: case OP_MONTY_ROUNDTRIP:
    case PL_RED_2P: case PL_CANON_SIGNED: case PL_CENTER_SIGNED: case PL_MHALVE: case PL_MDOUBLE: case PL_MDIV2: case PL_MDIV3:
    case PL_MDIV4: case PL_MDIV8: case PL_MDIV27: case PL_SBOX7: case PL_IDENTITY:
        a = 1; break;
    case OP_MMUL_LAZY: case OP_MMUL: case OP_MADD: case OP_MSUB: case OP_SMML: case OP_SMRED64: case OP_MRED64: case OP_SBOX7_RCS:
    case OP_SBOX7_RC: case OP_BITREV32:
        a = 2; break;
    case OP_MPOW: a = 3; break;
    case OP_LAZYACC: a = 5; break;
    case OP_EXT_ADD: case OP_EXT_SUB: case OP_EXT_MUL: a = 8; o = 4; break;
    case OP_EXT_MUL_BASE: a = 5; o = 4; break;
    case OP_EXT_FROBENIUS: case OP_EXT_INV: case OP_EXT_NEG: case OP_EXT_SQR: a = 4; o = 4; break;
    case OP_EXT_POW: a = 6; o = 4; break;
    case OP_P2_EXTERNAL: case OP_P2_INTERNAL: case OP_P2_PERMUTE: a = 16; o = 16; break;
    case OP_P2_COMPRESS: a = 16; o = 8; break;
    case OP_P2_HASH_SLICE: a = 1 + HASH_SLICE_MAX; o = 8; break;
    default: return false;
    }
    *arity = a;
    *outw = o;
    return true;
}

// ---- the plain forms: 64-bit `%` arithmetic, nothing from the headers but the constant P -------------------------------------
constexpr uint32_t plain_mulmod(uint64_t a, uint64_t b) { return (uint32_t)((a % P) * (b % P) % P); }
constexpr uint32_t plain_half_pow(int k) {   // 2^-k mod p, a compile-time constant wherever it is used
    uint32_t r = 1;
    for (int i = 0; i < k; i++) r = plain_mulmod(r, (P + 1u) / 2u);
    return r;
}
constexpr uint32_t plain_rinv6() {   // (2^-32)^6 mod p
    const uint32_t s = plain_mulmod(plain_half_pow(32), plain_half_pow(32));
    return plain_mulmod(plain_mulmod(s, s), s);
}
PROBE_HD static inline uint32_t plain(uint32_t op, uint32_t x) {
    constexpr uint32_t H1 = plain_half_pow(1), H2 = plain_half_pow(2), H3 = plain_half_pow(3), H4 = plain_half_pow(4), H8 = plain_half_pow(8),
                       H27 = plain_half_pow(27), RINV6 = plain_rinv6();
    switch (op) {
    case PL_RED_2P: return (uint64_t)x < 2ull * P ? (uint32_t)((uint64_t)x % P) : x - P;   // above 2p: the documented x - p
    case PL_CANON_SIGNED: return (uint32_t)((((int64_t)(int32_t)x % (int64_t)P) + (int64_t)P) % (int64_t)P);
    case PL_CENTER_SIGNED: return 2ull * x > (uint64_t)P ? (uint32_t)(int32_t)((int64_t)x - (int64_t)P) : x;
    case PL_MHALVE: return (uint32_t)((uint64_t)x * H1 % P);
    case PL_MDOUBLE: return (uint32_t)(2ull * x % P);
    case PL_MDIV2: return (uint32_t)((uint64_t)x * H2 % P);
    case PL_MDIV3: return (uint32_t)((uint64_t)x * H3 % P);
    case PL_MDIV4: return (uint32_t)((uint64_t)x * H4 % P);
    case PL_MDIV8: return (uint32_t)((uint64_t)x * H8 % P);
    case PL_MDIV27: return (uint32_t)((uint64_t)x * H27 % P);
    case PL_SBOX7: {   // Montgomery x^7: x^7 * (2^-32)^6 mod p
        const uint64_t x1 = (uint64_t)x % P, x2 = x1 * x1 % P, x4 = x2 * x2 % P, x6 = x4 * x2 % P, x7 = x6 * x1 % P;
        return (uint32_t)(x7 * RINV6 % P);
    }
    default: return (uint32_t)((uint64_t)x % P);   // PL_IDENTITY on [0, p)
    }
}

PROBE_HD static uint64_t u64_of(const uint32_t* w) { return (uint64_t)w[0] | ((uint64_t)w[1] << 32); }
PROBE_HD static Ext ext_of(const uint32_t* w) { return Ext{{w[0], w[1], w[2], w[3]}}; }
PROBE_HD static void put_ext(uint32_t* o, const Ext& e) {
    for (int i = 0; i < 4; i++) o[i] = e.c[i];
}

// one operation on one item: `in` holds arity(op) words, `out` takes outw(op) words
PROBE_HD static void apply_one(uint32_t op, const uint32_t* in, uint32_t* out) {
    uint32_t s[16];
    switch (op) {
    case OP_RED_2P: out[0] = red_2p(in[0]); break;
    case OP_MMUL_LAZY: out[0] = mmul_lazy(in[0], in[1]); break;
    case OP_MMUL: out[0] = mmul(in[0], in[1]); break;
    case OP_MADD: out[0] = madd(in[0], in[1]); break;
    case OP_MSUB: out[0] = msub(in[0], in[1]); break;
    case OP_MNEG: out[0] = mneg(in[0]); break;
    case OP_SMML: out[0] = (uint32_t)smml((int32_t)in[0], (int32_t)in[1]); break;
    case OP_CANON_SIGNED: out[0] = canon_signed((int32_t)in[0]); break;
    case OP_CENTER_SIGNED: out[0] = (uint32_t)center_signed(in[0]); break;
    case OP_SMRED64: out[0] = (uint32_t)smred64((int64_t)u64_of(in)); break;
    case OP_CANON_SIGNED_WIDE: out[0] = canon_signed_wide((int32_t)in[0]); break;
    case OP_MRED64: out[0] = mred64(u64_of(in)); break;
    case OP_LAZYACC: {   // in[4] times: add_group(t0), add_group(t1); then reduce
        LazyAcc acc;
        const uint64_t t0 = u64_of(in), t1 = u64_of(in + 2);
        const uint32_t reps = in[4];
        for (uint32_t k = 0; k < reps; k++) {
            acc.add_group(t0);
            acc.add_group(t1);
        }
        out[0] = acc.reduce();
        break;
    }
    case OP_TO_MONTY: out[0] = to_monty(in[0]); break;
    case OP_FROM_MONTY: out[0] = from_monty(in[0]); break;
    case OP_MONTY_ROUNDTRIP: out[0] = from_monty(to_monty(in[0])); break;
    case OP_MPOW: out[0] = mpow(in[0], u64_of(in + 1)); break;
    case OP_MINV: out[0] = minv(in[0]); break;
    case OP_EXT_ADD: put_ext(out, ext_add(ext_of(in), ext_of(in + 4))); break;
    case OP_EXT_SUB: put_ext(out, ext_sub(ext_of(in), ext_of(in + 4))); break;
    case OP_EXT_MUL: put_ext(out, ext_mul(ext_of(in), ext_of(in + 4))); break;
    case OP_EXT_MUL_BASE: put_ext(out, ext_mul_base(ext_of(in), in[4])); break;
    case OP_EXT_FROBENIUS: put_ext(out, ext_frobenius(ext_of(in))); break;
    case OP_EXT_INV: put_ext(out, ext_inv(ext_of(in))); break;
    case OP_EXT_NEG: put_ext(out, ext_neg(ext_of(in))); break;
    case OP_EXT_SQR: put_ext(out, ext_sqr(ext_of(in))); break;
    case OP_EXT_POW: put_ext(out, ext_pow(ext_of(in), u64_of(in + 4))); break;
    case OP_MDOUBLE: out[0] = mdouble(in[0]); break;
    case OP_MHALVE: out[0] = mhalve(in[0]); break;
    case OP_MDIV2: out[0] = mdiv_pow2<2>(in[0]); break;
    case OP_MDIV3: out[0] = mdiv_pow2<3>(in[0]); break;
    case OP_MDIV4: out[0] = mdiv_pow2<4>(in[0]); break;
    case OP_MDIV8: out[0] = mdiv_pow2<8>(in[0]); break;
    case OP_MDIV27: out[0] = mdiv_pow2<27>(in[0]); break;
    case OP_SBOX7: out[0] = sbox7(in[0]); break;
    case OP_SBOX7_RCS: out[0] = sbox7_rcs(in[0], in[1]); break;
    case OP_SBOX7_RC: out[0] = sbox7_rc(in[0], in[1]); break;
    case OP_P2_EXTERNAL: case OP_P2_INTERNAL: case OP_P2_PERMUTE:
        for (int i = 0; i < 16; i++) s[i] = in[i];
        if (op == OP_P2_EXTERNAL) p2_external_linear(s);
        else if (op == OP_P2_INTERNAL) p2_internal_linear(s);
        else poseidon2_permute(s);
        for (int i = 0; i < 16; i++) out[i] = s[i];
        break;
    case OP_TWO_ADIC_GEN: out[0] = two_adic_generator(in[0]); break;
    case OP_BITREV32: out[0] = bitrev32(in[0], in[1]); break;
    case OP_P2_COMPRESS: p2_compress(in, in + 8, out); break;
    case OP_P2_HASH_SLICE: p2_hash_slice(in + 1, in[0], out); break;
    default: out[0] = plain(op, in[0]); break;
    }
}

// operands the probe itself refuses: loop counts and lengths that would run long or read past the item
static bool item_ok(uint32_t op, const uint32_t* in) {
    if (op == OP_LAZYACC) return in[4] <= LAZYACC_MAX_REPS;
    if (op == OP_P2_HASH_SLICE) return in[0] <= HASH_SLICE_MAX;
    if (op == OP_TWO_ADIC_GEN) return in[0] <= 27;
    if (op == OP_BITREV32) return in[1] <= 32;
    return true;
}

struct Exhaustive {
    uint32_t fast_op, plain_op, stride, bias;
    uint64_t start, count;
};
// the pairs an exhaustive job may name: each gets a loop of its own, with the operation known at compile time
#define EXHAUSTIVE_PAIRS(X)                                                                                                        \
    X(OP_RED_2P, PL_RED_2P) X(OP_CANON_SIGNED, PL_CANON_SIGNED) X(OP_CENTER_SIGNED, PL_CENTER_SIGNED) X(OP_MHALVE, PL_MHALVE)      \
    X(OP_MDOUBLE, PL_MDOUBLE) X(OP_MDIV2, PL_MDIV2) X(OP_MDIV3, PL_MDIV3) X(OP_MDIV4, PL_MDIV4) X(OP_MDIV8, PL_MDIV8)              \
    X(OP_MDIV27, PL_MDIV27) X(OP_SBOX7, PL_SBOX7) X(OP_MONTY_ROUNDTRIP, PL_IDENTITY)

template <uint32_t OP>
PROBE_HD static inline uint32_t unary(uint32_t x) {
    if constexpr (OP == OP_RED_2P) return red_2p(x);
    else if constexpr (OP == OP_CANON_SIGNED) return canon_signed((int32_t)x);
    else if constexpr (OP == OP_CENTER_SIGNED) return (uint32_t)center_signed(x);
    else if constexpr (OP == OP_MHALVE) return mhalve(x);
    else if constexpr (OP == OP_MDOUBLE) return mdouble(x);
    else if constexpr (OP == OP_MDIV2) return mdiv_pow2<2>(x);
    else if constexpr (OP == OP_MDIV3) return mdiv_pow2<3>(x);
    else if constexpr (OP == OP_MDIV4) return mdiv_pow2<4>(x);
    else if constexpr (OP == OP_MDIV8) return mdiv_pow2<8>(x);
    else if constexpr (OP == OP_MDIV27) return mdiv_pow2<27>(x);
    else if constexpr (OP == OP_SBOX7) return sbox7(x);
    else if constexpr (OP == OP_MONTY_ROUNDTRIP) return from_monty(to_monty(x));
    else return plain(OP, x);
}

#if defined(__HIPCC__)
#define HIP_OK(e)                                                                                  \
    do {                                                                                           \
        hipError_t err_ = (e);                                                                     \
        if (err_ != hipSuccess) {                                                                  \
            fprintf(stderr, "field_probe: %s: %s\n", #e, hipGetErrorString(err_));                 \
            exit(3);                                                                               \
        }                                                                                          \
    } while (0)

__global__ void k_apply(uint32_t op, uint32_t arity, uint32_t outw, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) apply_one(op, in + (size_t)i * arity, out + (size_t)i * outw);
}

// res[0] = mismatches, res[1] = smallest mismatching index
template <uint32_t FAST, uint32_t PLAIN>
__global__ void k_exhaustive(Exhaustive e, unsigned long long* res) {
    unsigned long long bad = 0, first = ~0ull;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < e.count; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t index = e.start + k * e.stride;
        const uint32_t x = (uint32_t)(index - e.bias);
        if (unary<FAST>(x) != unary<PLAIN>(x)) {
            bad++;
            if (index < first) first = index;
        }
    }
    if (bad) {
        atomicAdd(&res[0], bad);
        atomicMin(&res[1], first);
    }
}

static void run_apply(uint32_t op, uint32_t arity, uint32_t outw, const uint32_t* in, uint32_t* out, uint32_t n) {
    if (n == 0) return;
    uint32_t *d_in, *d_out;
    HIP_OK(hipMalloc(&d_in, (size_t)n * arity * 4));
    HIP_OK(hipMalloc(&d_out, (size_t)n * outw * 4));
    HIP_OK(hipMemcpy(d_in, in, (size_t)n * arity * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_apply, dim3((n + 127) / 128), dim3(128), 0, 0, op, arity, outw, d_in, d_out, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, d_out, (size_t)n * outw * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));
}

static bool run_exhaustive(const Exhaustive& e, uint64_t* bad, uint64_t* first) {
    bool known = false;
#define X(F, PL) known = known || (e.fast_op == F && e.plain_op == PL);
    EXHAUSTIVE_PAIRS(X)
#undef X
    if (!known) return false;
    unsigned long long h[2] = {0, ~0ull}, *d;
    HIP_OK(hipMalloc(&d, sizeof h));
    HIP_OK(hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice));
    switch (e.fast_op) {
#define X(F, PL)                                                                                   \
    case F:                                                                                        \
        hipLaunchKernelGGL((k_exhaustive<F, PL>), dim3(4096), dim3(256), 0, 0, e, d);              \
        break;
        EXHAUSTIVE_PAIRS(X)
#undef X
    default: break;
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d));
    *bad = h[0];
    *first = h[1];
    return true;
}
#else
static void run_apply(uint32_t op, uint32_t arity, uint32_t outw, const uint32_t* in, uint32_t* out, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) apply_one(op, in + (size_t)i * arity, out + (size_t)i * outw);
}

template <uint32_t FAST, uint32_t PLAIN>
static void exhaustive_loop(const Exhaustive& e, uint64_t* bad, uint64_t* first) {
    for (uint64_t k = 0; k < e.count; k++) {
        const uint64_t index = e.start + k * e.stride;
        const uint32_t x = (uint32_t)(index - e.bias);
        if (unary<FAST>(x) != unary<PLAIN>(x)) {
            ++*bad;
            if (index < *first) *first = index;
        }
    }
}

static bool run_exhaustive(const Exhaustive& e, uint64_t* bad, uint64_t* first) {
    *bad = 0;
    *first = ~0ull;
    switch (e.fast_op) {
#define X(F, PL)                                                                                   \
    case F:                                                                                        \
        if (e.plain_op != PL) return false;                                                        \
        exhaustive_loop<F, PL>(e, bad, first);                                                     \
        return true;
        EXHAUSTIVE_PAIRS(X)
#undef X
    default: return false;
    }
}
#endif

// elapsed time of every job on stderr: a slow or stuck step is named in the test's failure message
static double now_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int fail(const char* what) {
    fprintf(stderr, "field_probe: %s\n", what);
    return 2;
}

int main(int argc, char** argv) {
    constexpr uint32_t MAGIC = 0x31425046u;
    if (argc != 3) return fail("usage: field_probe <operand file> <result file>");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail("cannot open the operand file");
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 8 || bytes % 4 != 0) return fail("operand file: bad size");
    std::vector<uint32_t> in((size_t)bytes / 4);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return fail("operand file: short read");
    fclose(f);
    if (in[0] != MAGIC) return fail("operand file: bad magic");
    const uint32_t n_jobs = in[1];
    std::vector<uint32_t> out = {MAGIC, n_jobs};
    size_t pos = 2;
    for (uint32_t j = 0; j < n_jobs; j++) {
        if (pos >= in.size()) return fail("operand file: truncated job list");
        const uint32_t kind = in[pos++];
        if (kind == 0) {
            if (in.size() - pos < 2) return fail("apply job: truncated header");
            const uint32_t op = in[pos], n = in[pos + 1];
            pos += 2;
            uint32_t arity, outw;
            if (!op_shape(op, &arity, &outw)) return fail("apply job: unknown operation");
            if (n > MAX_ITEMS || (size_t)n * arity > in.size() - pos) return fail("apply job: operands exceed the file");
            for (uint32_t i = 0; i < n; i++)
                if (!item_ok(op, &in[pos + (size_t)i * arity])) return fail("apply job: operand outside the probe's limits");
            const size_t at = out.size();
            out.resize(at + (size_t)n * outw);
            const double t0 = now_s();
            run_apply(op, arity, outw, in.data() + pos, out.data() + at, n);
            fprintf(stderr, "job %u: op %u, %u items: %.3f s\n", j, op, n, now_s() - t0);
            pos += (size_t)n * arity;
        } else if (kind == 1) {
            if (in.size() - pos < 8) return fail("exhaustive job: truncated");
            Exhaustive e;
            e.fast_op = in[pos], e.plain_op = in[pos + 1];
            e.start = u64_of(&in[pos + 2]), e.count = u64_of(&in[pos + 4]);
            e.stride = in[pos + 6], e.bias = in[pos + 7];
            pos += 8;
            uint32_t a1, o1, a2, o2;
            if (!op_shape(e.fast_op, &a1, &o1) || !op_shape(e.plain_op, &a2, &o2) || a1 != 1 || a2 != 1 || o1 != 1 || o2 != 1)
                return fail("exhaustive job: both operations must be unary");
            // every index start + k * stride (k < count) stays at or below 2^33, checked without a product that could wrap
            if (e.stride == 0 || e.start > (1ull << 33) || (e.count > 0 && e.count - 1 > ((1ull << 33) - e.start) / e.stride))
                return fail("exhaustive job: range too large");
            uint64_t bad, first;
            const double t0 = now_s();
            if (!run_exhaustive(e, &bad, &first)) return fail("exhaustive job: not one of the known (fast, plain) pairs");
            fprintf(stderr, "job %u: exhaustive %u vs %u, %llu operands: %.3f s\n", j, e.fast_op, e.plain_op, (unsigned long long)e.count, now_s() - t0);
            out.push_back((uint32_t)bad), out.push_back((uint32_t)(bad >> 32));
            out.push_back((uint32_t)first), out.push_back((uint32_t)(first >> 32));
        } else {
            return fail("unknown job kind");
        }
    }
    if (pos != in.size()) return fail("operand file: trailing words");
    FILE* g = fopen(argv[2], "wb");
    if (!g) return fail("cannot open the result file");
    if (fwrite(out.data(), 4, out.size(), g) != out.size()) return fail("result file: short write");
    fclose(g);
    return 0;
}
