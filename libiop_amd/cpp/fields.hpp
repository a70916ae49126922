// Plain field-element types for C++ callers that do not link libff: 8 raw bytes with the layout of libff::gf64, 16 with that of libff::gf128, 32 with that of libff::gf256, 24 raw bytes with the layout of libff::gf192 (three
// little-endian words, polynomial basis) / libff::edwards_Fr (three Montgomery limbs), 32 with that of libff::alt_bn128_Fr (four).
// They provide what the mirror asks of a FieldT — construction from an integer, ==, + — through the library's host helpers; a libiop
// integration uses libff's own types instead.
#pragma once
#include "iop.hpp"

namespace libiop_amd {

struct gf192_element {
    uint64_t w[3];
    gf192_element() : w{ 0, 0, 0 } {}
    explicit gf192_element(uint64_t v) : w{ v, 0, 0 } {}
    bool operator==(const gf192_element &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2]; }
    bool operator!=(const gf192_element &o) const { return !(*this == o); }
    gf192_element operator+(const gf192_element &o) const { gf192_element r; for (int i = 0; i < 3; ++i) r.w[i] = w[i] ^ o.w[i]; return r; }
    gf192_element &operator+=(const gf192_element &o) { for (int i = 0; i < 3; ++i) w[i] ^= o.w[i]; return *this; }
};
template<> struct field_kind<gf192_element> { static const field_subset_type type = affine_subspace_type; };

// 8 raw bytes with the layout of libff::gf64 (one little-endian word, polynomial basis, x^64 + x^4 + x^3 + x + 1)
struct gf64 {
    uint64_t w[1];
    gf64() : w{ 0 } {}
    explicit gf64(uint64_t v) : w{ v } {}
    bool operator==(const gf64 &o) const { return w[0] == o.w[0]; }
    bool operator!=(const gf64 &o) const { return !(*this == o); }
    gf64 operator+(const gf64 &o) const { return gf64(w[0] ^ o.w[0]); }
    gf64 &operator+=(const gf64 &o) { w[0] ^= o.w[0]; return *this; }
};
template<> struct field_kind<gf64> { static const field_subset_type type = affine_subspace_type; };

// 16 raw bytes with the layout of libff::gf128 (two little-endian words, polynomial basis, x^128 + x^7 + x^2 + x + 1)
struct gf128 {
    uint64_t w[2];
    gf128() : w{ 0, 0 } {}
    explicit gf128(uint64_t v) : w{ v, 0 } {}
    bool operator==(const gf128 &o) const { return w[0] == o.w[0] && w[1] == o.w[1]; }
    bool operator!=(const gf128 &o) const { return !(*this == o); }
    gf128 operator+(const gf128 &o) const { gf128 r; r.w[0] = w[0] ^ o.w[0]; r.w[1] = w[1] ^ o.w[1]; return r; }
    gf128 &operator+=(const gf128 &o) { w[0] ^= o.w[0]; w[1] ^= o.w[1]; return *this; }
};
template<> struct field_kind<gf128> { static const field_subset_type type = affine_subspace_type; };

// 32 raw bytes with the layout of libff::gf256 (four little-endian words, polynomial basis, x^256 + x^10 + x^5 + x^2 + 1)
struct gf256 {
    uint64_t w[4];
    gf256() : w{ 0, 0, 0, 0 } {}
    explicit gf256(uint64_t v) : w{ v, 0, 0, 0 } {}
    bool operator==(const gf256 &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    bool operator!=(const gf256 &o) const { return !(*this == o); }
    gf256 operator+(const gf256 &o) const { gf256 r; for (int i = 0; i < 4; ++i) r.w[i] = w[i] ^ o.w[i]; return r; }
    gf256 &operator+=(const gf256 &o) { for (int i = 0; i < 4; ++i) w[i] ^= o.w[i]; return *this; }
};
template<> struct field_kind<gf256> { static const field_subset_type type = affine_subspace_type; };

struct edwards_Fr_element {
    uint64_t w[3];
    edwards_Fr_element() : w{ 0, 0, 0 } {}
    explicit edwards_Fr_element(uint64_t v) { check(ops::edwards_Fr.from_uint(v, w)); }
    bool operator==(const edwards_Fr_element &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2]; }
    bool operator!=(const edwards_Fr_element &o) const { return !(*this == o); }
    edwards_Fr_element operator+(const edwards_Fr_element &o) const { edwards_Fr_element r; check(ops::edwards_Fr.host_add(w, o.w, r.w)); return r; }
};
template<> struct field_kind<edwards_Fr_element> { static const field_subset_type type = multiplicative_coset_type; };

// 32 raw bytes with the layout of libff::alt_bn128_Fr (four Montgomery limbs, R = 2^256)
struct alt_bn128_Fr_element {
    uint64_t w[4];
    alt_bn128_Fr_element() : w{ 0, 0, 0, 0 } {}
    explicit alt_bn128_Fr_element(uint64_t v) { check(ops::alt_bn128_Fr.from_uint(v, w)); }
    bool operator==(const alt_bn128_Fr_element &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    bool operator!=(const alt_bn128_Fr_element &o) const { return !(*this == o); }
    alt_bn128_Fr_element operator+(const alt_bn128_Fr_element &o) const { alt_bn128_Fr_element r; check(ops::alt_bn128_Fr.host_add(w, o.w, r.w)); return r; }
};
template<> struct field_kind<alt_bn128_Fr_element> { static const field_subset_type type = multiplicative_coset_type; };

} // namespace libiop_amd
