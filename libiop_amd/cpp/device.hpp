// Host scalars of FieldT and device-resident storage for C++ callers of the C ABI: field_host<FieldT> (per-proof constants),
// device_array<T> / device_vector<FieldT> (pooled HBM blocks, iopx_pool_alloc) — the storage behind oracle<FieldT>, where the reference
// has std::vector<FieldT> on the heap (libiop/iop/oracles.hpp:22-52).
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <set>

#include "libiop_amd.hpp"

namespace libiop_amd {

// ---- host scalars of FieldT (per-proof constants only) --------------------------------------------------------------------------
// One body for every field, written against the table of field_ops.hpp: gf192 keeps its branches (xor, the subspace forms of Z_S),
// everything else is the field's entry (Z_S on the host included).  A size / kind the table does not have fails to compile.
template<typename FieldT>
struct field_host {
    typedef ops::field<sizeof(FieldT), field_kind<FieldT>::type == affine_subspace_type> table;
    typedef ops::prime_field_ops P;
    static const std::size_t WORDS = sizeof(FieldT) / 8;
    template<typename Slot> static auto entry(Slot slot, const char *op) { return ops::entry<table>(slot, op); }
    template<typename Fn> static FieldT binary(Fn fn, const FieldT &a, const FieldT &b) { uint64_t w[WORDS]; check(fn(detail::words(&a), detail::words(&b), w)); return from_words(w); }

    static bool additive() { return table::additive; }
    static FieldT from_words(const uint64_t *w) { FieldT r; std::memcpy((void *)&r, w, sizeof(FieldT)); return r; }
    static FieldT zero() { const uint64_t w[WORDS] = {}; return from_words(w); }
    static FieldT from_uint(uint64_t v)
    {
        uint64_t w[WORDS] = { v };
        if (!additive()) check(entry(&P::from_uint, "from_uint")(v, w));
        return from_words(w);
    }
    static FieldT one() { return from_uint(1); }
    static bool is_zero(const FieldT &a) { uint64_t any = 0; for (std::size_t i = 0; i < WORDS; ++i) any |= detail::words(&a)[i]; return any == 0; }
    static FieldT add(const FieldT &a, const FieldT &b)
    {
        if (!additive()) return binary(entry(&P::host_add, "add"), a, b);
        uint64_t w[WORDS];
        for (std::size_t i = 0; i < WORDS; ++i) w[i] = detail::words(&a)[i] ^ detail::words(&b)[i];
        return from_words(w);
    }
    static FieldT sub(const FieldT &a, const FieldT &b) { return additive() ? add(a, b) : binary(entry(&P::host_sub, "sub"), a, b); }
    static FieldT mul(const FieldT &a, const FieldT &b) { return binary(entry(&P::host_mul, "mul"), a, b); }
    static FieldT pow(const FieldT &a, uint64_t e)
    {
        if (!additive()) { uint64_t w[WORDS]; check(entry(&P::host_pow, "pow")(detail::words(&a), e, w)); return from_words(w); }
        FieldT r = one(), b = a;
        for (; e; e >>= 1) { if (e & 1) r = mul(r, b); b = mul(b, b); }
        return r;
    }
    static FieldT neg(const FieldT &a) { return sub(zero(), a); }
    static FieldT inverse(const FieldT &a) { uint64_t w[WORDS]; check(entry(&P::host_inverse, "inverse")(detail::words(&a), w)); return from_words(w); }
    // Over gf64, gf128 and gf256 only the head route and the Fractal prover ask for Z_S on the host, and they sit behind IOPX_GFX_HEAD_EVAL and
    // IOPX_GFX_FRACTAL / IOPX_GFX_FRACTAL_WIDE: with the three options unset the two subspace forms below are refused as before any of them existed
    // (nothing observable changes); with one set they go through the field's vanishing_host slot
    static bool subspace_host_forms()
    {
        return WORDS == 3 || iopx_get_option("IOPX_GFX_HEAD_EVAL", 0) != 0 || iopx_get_option("IOPX_GFX_FRACTAL", 0) != 0 ||
               iopx_get_option("IOPX_GFX_FRACTAL_WIDE", 0) != 0;
    }
    // Z_S(x) for the domain S (vanishing_polynomial::evaluation_at_point): the linearized polynomial of the subspace through the
    // library's host helper / x^|S| - shift^|S| (vanishing_polynomial.tcc:14-25)
    static FieldT vanishing_eval(const field_subset<FieldT> &S, const FieldT &x)
    {
        if (S.type() == affine_subspace_type) {
            if (!subspace_host_forms()) ops::missing("vanishing_eval", table::vec->name);
            uint64_t w[WORDS];
            const FieldT shift = S.shift();
            check(entry(&ops::subspace_ops::vanishing_host, "vanishing_eval")(detail::words(S.basis().data()), S.dimension(), detail::words(&shift), detail::words(&x), w, nullptr));
            return from_words(w);
        }
        return sub(pow(x, S.num_elements()), pow(S.shift(), S.num_elements()));
    }
    // (DZ_S)(x): the linear coefficient for subspaces (vanishing_polynomial.tcc:63-72), |S| x^(|S| - 1) for cosets (:57-62)
    static FieldT vanishing_derivative(const field_subset<FieldT> &S, const FieldT &x)
    {
        if (S.type() == affine_subspace_type) {
            if (!subspace_host_forms()) ops::missing("vanishing_derivative", table::vec->name);
            uint64_t w[WORDS];
            const FieldT shift = S.shift();
            check(entry(&ops::subspace_ops::vanishing_host, "vanishing_derivative")(detail::words(S.basis().data()), S.dimension(), detail::words(&shift), detail::words(&x), nullptr, w));
            return from_words(w);
        }
        return mul(from_uint(S.num_elements()), pow(x, S.num_elements() - 1));
    }
    // membership of x in S: standard-basis subspaces (x + shift below 2^dim) / (x / shift)^|S| = 1
    static bool element_in_domain(const field_subset<FieldT> &S, const FieldT &x)
    {
        if (S.type() == affine_subspace_type) {
            if (!S.subspace().is_standard_basis()) throw std::logic_error("membership test for a non-standard basis");
            const FieldT v = add(x, S.shift());
            const uint64_t *w = detail::words(&v);
            for (std::size_t i = 1; i < WORDS; ++i) if (w[i]) return false;
            return S.dimension() >= 64 || w[0] < ((uint64_t)1 << S.dimension());
        }
        const FieldT r = pow(mul(x, inverse(S.shift())), S.num_elements());
        const FieldT o = one();
        return std::memcmp(&r, &o, sizeof(FieldT)) == 0;
    }
    static std::size_t soundness_bits() { return table::vec->soundness_bits; }
};

// the field's C entry for one table slot, e.g. field_entry<FieldT>(&ops::vector_ops::mul, "mul")(a, b, out, count)
template<typename FieldT, typename Slot> inline auto field_entry(Slot slot, const char *op) { return field_host<FieldT>::entry(slot, op); }
// its selection, for the domain-shaped operations: ops::rowcheck<field_of<FieldT>>(...)
template<typename FieldT> using field_of = typename field_host<FieldT>::table;

// ---- device memory -----------------------------------------------------------------------------------------------------------------
namespace detail {
struct pooled_block {
    void *p = nullptr;
    explicit pooled_block(std::size_t bytes) { check(iopx_pool_alloc(&p, bytes)); }
    pooled_block(const pooled_block &) = delete;
    pooled_block &operator=(const pooled_block &) = delete;
    ~pooled_block() { if (p) iopx_pool_free(p); }
};
} // namespace detail

// `count` elements of elem_bytes in HBM; copies share the block, slice() is a view
template<typename T>
class device_array {
    std::shared_ptr<detail::pooled_block> block_;
    std::size_t offset_ = 0, size_ = 0;
public:
    device_array() {}
    explicit device_array(std::size_t count) : block_(std::make_shared<detail::pooled_block>((count ? count : 1) * sizeof(T))), size_(count) {}
    std::size_t size() const { return size_; }
    bool empty() const { return size_ == 0; }
    T *data() const { return block_ ? reinterpret_cast<T *>(block_->p) + offset_ : nullptr; }
    device_array slice(std::size_t begin, std::size_t count) const
    {
        if (begin + count > size_) throw std::invalid_argument("device_array::slice out of range");
        device_array r;
        r.block_ = block_; r.offset_ = offset_ + begin; r.size_ = count;
        return r;
    }
    static device_array from_host(const T *src, std::size_t count)
    {
        device_array r(count);
        if (count) check(iopx_memcpy_h2d(r.data(), src, count * sizeof(T)));
        return r;
    }
    static device_array from_host(const std::vector<T> &v) { return from_host(v.data(), v.size()); }
    std::vector<T> to_host(std::size_t count = (std::size_t)-1) const
    {
        if (count == (std::size_t)-1) count = size_;
        if (count > size_) throw std::invalid_argument("device_array::to_host out of range");
        std::vector<T> out(count);
        if (count) check(iopx_memcpy_d2h(out.data(), data(), count * sizeof(T)));
        return out;
    }
    void fill_zero() const { if (size_) check(iopx_memset_dev(data(), 0, size_ * sizeof(T))); }
    void copy_from(const device_array &src) const
    {
        if (src.size() != size_) throw std::invalid_argument("device_array::copy_from: size mismatch");
        if (size_) check(iopx_memcpy_d2d(data(), src.data(), size_ * sizeof(T)));
    }
};

template<typename FieldT>
class device_vector : public device_array<FieldT> {
public:
    device_vector() {}
    explicit device_vector(std::size_t count) : device_array<FieldT>(count) {}
    device_vector(const device_array<FieldT> &a) : device_array<FieldT>(a) {}
    uint64_t *words() const { return reinterpret_cast<uint64_t *>(this->data()); }
    device_vector slice(std::size_t begin, std::size_t count) const { return device_vector(device_array<FieldT>::slice(begin, count)); }
};

} // namespace libiop_amd
