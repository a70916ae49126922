// Host-side description of the two prime fields of the multiplicative-coset code (fft_mul.hip, ldt_reducer.hip): the host element
// type, its size, the field facts the argument checks and the subgroup generators need, and whether two-level power tables are cached.
#pragma once
#include <cstddef>
#include <cstdint>
#include "bn254_host.h"
#include "fp3_host.h"

namespace iopx {

struct FpField {
    typedef hfp3 H;
    static const int WORDS = 3;
    static const size_t BYTES = 24;                 // per element
    static constexpr const char *NAME = "edwards_Fr";
    static const int TWO_ADICITY = 31;
    static const uint64_t GENERATOR = 19;           // libff edwards_Fr::multiplicative_generator (recalled)
    static const bool CACHE_TABLES = true;          // two-level power tables are kept in fft_mul.hip's g_pow_tables
};

struct BnField {
    typedef hbn H;
    static const int WORDS = 4;
    static const size_t BYTES = 32;
    static constexpr const char *NAME = "alt_bn128 Fr";
    static const int TWO_ADICITY = 28;
    static const uint64_t GENERATOR = 5;            // libff alt_bn128_Fr::multiplicative_generator
    static const bool CACHE_TABLES = false;         // built per call (caching them is a separate, measured change)
};

} // namespace iopx
