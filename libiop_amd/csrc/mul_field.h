// Host-side description of the two prime fields of the multiplicative-coset code (fft_mul.hip, ldt_reducer.hip): the host element
// type, its size, the field facts the argument checks and the subgroup generators need, and whether two-level power tables are cached.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "bn254_host.h"
#include "fp3_host.h"

namespace iopx {

// GF(2^192), for the host functions that serve all three fields (*_common in virtual_oracles.hip, encoded_ops.hip, fractal_ops.hip):
// constants go to the device as they are
struct Gf192Field {
    static const int WORDS = 3;
    static const size_t BYTES = 24;
    static const bool PRIME = false;
};

// `num` host elements in the form the field's kernels multiply by: table form over a prime field, unchanged over GF(2^192)
template<class F>
static inline void multiplier_words(const uint64_t *src, size_t num, uint64_t *dst)
{
    if constexpr (F::PRIME) {
        for (size_t i = 0; i < num; ++i) { const typename F::H t = F::H::from_words(src + F::WORDS * i).table_form(); memcpy(dst + F::WORDS * i, t.w, F::BYTES); }
    } else {
        memcpy(dst, src, num * F::BYTES);
    }
}

struct FpField {
    typedef hfp3 H;
    static const int WORDS = 3;
    static const size_t BYTES = 24;                 // per element
    static constexpr const char *NAME = "edwards_Fr";
    static const int TWO_ADICITY = 31;
    static const uint64_t GENERATOR = 19;           // libff edwards_Fr::multiplicative_generator (recalled)
    static const bool CACHE_TABLES = true;          // two-level power tables are kept in fft_mul.hip's g_pow_tables
    static const uint64_t TABLE_FACTOR = 2048;      // H::table_form() multiplies by it: device radix 2^203 against the stored 2^192
    static const bool PRIME = true;                 // multipliers are uploaded in table form
    static const bool RAW_INPUTS = false;           // data operands are canonical words
};

struct BnField {
    typedef hbn H;
    static const int WORDS = 4;
    static const size_t BYTES = 32;
    static constexpr const char *NAME = "alt_bn128 Fr";
    static const int TWO_ADICITY = 28;
    static const uint64_t GENERATOR = 5;            // libff alt_bn128_Fr::multiplicative_generator
    static const bool CACHE_TABLES = false;         // built per call (caching them is a separate, measured change)
    static const uint64_t TABLE_FACTOR = 32;        // device radix 2^261 against the stored 2^256
    static const bool PRIME = true;
    static const bool RAW_INPUTS = true;            // data operands may be any 256-bit word, outputs are canonical: a copy must reduce too
};

} // namespace iopx
