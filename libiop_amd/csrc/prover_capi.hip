// The Aurora, Fractal and FRI-only provers behind the C ABI: iopx_aurora_* / iopx_fractal_* / iopx_fri_snark_* (include/libiop_amd.h).
//
// The orchestration is the C++ surface of libiop_amd/cpp/aurora.hpp — aurora_snark_prover<FieldT>(cs, primary, auxiliary, params),
// the signature of libiop/snark/aurora_snark.tcc:120-146 — instantiated for the four accelerated fields and wrapped in plain C types, so
// that a caller without a C++ toolchain (the ctypes binding, bench.py) reaches the native prover too.  Host-only code: no kernels here.
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "../cpp/aurora.hpp"
#include "../cpp/fractal.hpp"
#include "../cpp/fri.hpp"
#include "../cpp/fields.hpp"
#include "runtime.h"

namespace {

using namespace libiop_amd;

// The BCS layer of libiop_amd/cpp/iop.hpp works with 32-byte BLAKE2b digests — hashchain state, roots, paths, proof of work — which is
// digest_len_bytes = 2 * security_parameter / 8 of the reference (blake2b.tcc:15, hash_enum.tcc) for security_parameter = 128 only; any
// other value would run and return a transcript the reference does not produce, so it is refused.
void require_supported_security(size_t security_parameter)
{
    if (security_parameter != 128)
        throw std::invalid_argument("security_parameter " + std::to_string(security_parameter) + " is not supported: the native BCS layer uses 32-byte digests "
                                    "(digest_len_bytes = 2 * security_parameter / 8 for security_parameter = 128)");
}

struct InstanceBase {
    virtual ~InstanceBase() {}
    // comm: the communicator the codeword-domain vectors are distributed over (libiop_amd/cpp/dist.hpp); null = one GPU
    virtual std::string prove(iopx_comm *comm, int bcs_hash_type, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) = 0;
    virtual size_t num_constraints() const = 0;
    virtual std::vector<std::string> fractal_index(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) = 0;
    virtual std::string fractal_prove(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) = 0;
};

template<typename F>
struct Instance : InstanceBase {
    r1cs_constraint_system<F> cs;
    std::vector<F> primary, auxiliary;
    device_vector<F> d_assignment;          // (1, primary, auxiliary), resident in HBM

    void finish()
    {
        cs.prepare_device();
        std::vector<F> z(1, field_host<F>::one());
        z.insert(z.end(), primary.begin(), primary.end());
        z.insert(z.end(), auxiliary.begin(), auxiliary.end());
        d_assignment = device_vector<F>(device_array<F>::from_host(z));
    }
    // the Fractal prover index (twelve index oracles, their tree, their evaluations over the index domain) for one parameter set
    std::unique_ptr<bcs_prover_index<F>> index;
    size_t index_params[3] = { 0, 0, 0 };
    iopx_comm *index_comm = nullptr;        // the index holds this rank's part of the twelve index oracles: it belongs to one communicator

    size_t num_constraints() const override { return cs.num_constraints(); }
    static constexpr bool binary = field_kind<F>::type == affine_subspace_type;      // 32 bytes are alt_bn128 Fr or gf256: the kind tells them apart
    static constexpr bool bn128 = !binary && sizeof(F) == 32;     // alt_bn128 Fr: Aurora only, on one GPU
    static constexpr bool gf64 = binary && sizeof(F) == 8;        // gf64: Aurora, and Fractal behind IOPX_GFX_FRACTAL; on one GPU, BLAKE2b
    static constexpr bool gf128 = binary && sizeof(F) == 16;      // gf128, gf256: as gf64, with Fractal behind IOPX_GFX_FRACTAL_WIDE
    static constexpr bool gf256 = binary && sizeof(F) == 32;
    static constexpr bool gfx = gf128 || gf256;
    static const char *gfx_name() { return gf128 ? "gf128" : "gf256"; }
    static const char *subspace_name() { return gf64 ? "gf64" : gfx_name(); }
    // gf64, gf128, gf256: Fractal behind an option (default 0, looked up per call: unset, the refusal of before the prover was built) — IOPX_GFX_FRACTAL
    // for gf64, IOPX_GFX_FRACTAL_WIDE for gf128 and gf256, neither speaking for the other — on one GPU; a codeword domain past the transforms' cap is
    // refused before any device work
    void subspace_fractal(const char *entry, iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) const
    {
        const std::string name = subspace_name();
        if (iopx_get_option(gf64 ? "IOPX_GFX_FRACTAL" : "IOPX_GFX_FRACTAL_WIDE", 0) == 0) throw std::invalid_argument(std::string(entry) + ": there is no Fractal prover over " + name);
        if (comm) throw std::invalid_argument(name + " has no distributed prover: pass no communicator");
        require_supported_security(security_parameter);
        const fractal_snark_parameters<F> params(cs, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        const size_t cap = gf64 ? IOPX_GF64_MAX_DOMAIN_DIM : IOPX_GFX_MAX_DOMAIN_DIM;
        if (params.codeword_domain_dim_ > cap)
            throw std::invalid_argument("codeword domain dimension " + std::to_string(params.codeword_domain_dim_) + ": the " + name + " transforms take domains of dimension up to " +
                                        std::to_string(cap));
    }
    std::vector<std::string> fractal_index(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) override
    {
        if constexpr (bn128) throw std::invalid_argument("iopx_fractal_index: there is no Fractal prover over alt_bn128 Fr");
        else if constexpr (gf64 || gfx) return subspace_fractal("iopx_fractal_index", comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter), fractal_index_(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        else return fractal_index_(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
    }
    std::string fractal_prove(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) override
    {
        if constexpr (bn128) throw std::invalid_argument("iopx_fractal_prove: there is no Fractal prover over alt_bn128 Fr");
        else if constexpr (gf64 || gfx) return subspace_fractal("iopx_fractal_prove", comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter), fractal_prove_(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        else return fractal_prove_(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
    }
    std::vector<std::string> fractal_index_(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter)
    {
        require_supported_security(security_parameter);
        const dist::scope bound(comm);
        const fractal_snark_parameters<F> params(cs, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        index.reset();                                           // a failed indexer leaves no index behind, rather than the previous one under a new label
        index_params[0] = index_params[1] = index_params[2] = 0;
        auto made = fractal_snark_indexer<F>(cs, params);
        index.reset(new bcs_prover_index<F>(std::move(made.first)));
        index_comm = comm;
        index_params[0] = security_parameter; index_params[1] = RS_extra_dimensions; index_params[2] = FRI_localization_parameter;
        return made.second.index_MT_roots_;
    }
    std::string fractal_prove_(iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter)
    {
        require_supported_security(security_parameter);
        if (index && index_comm != comm) throw std::logic_error("iopx_fractal_prove: the index was built for another communicator");
        const dist::scope bound(comm);
        if (!index || index_params[0] != security_parameter || index_params[1] != RS_extra_dimensions || index_params[2] != FRI_localization_parameter)
            throw std::logic_error("iopx_fractal_prove: no index for these parameters (call iopx_fractal_index first)");
        const fractal_snark_parameters<F> params(cs, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        return fractal_snark_prover_serialized<F>(*index, cs, primary, auxiliary, params, &d_assignment);
    }
    std::string prove(iopx_comm *comm, int bcs_hash_type, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter) override
    {
        if (bcs_hash_type != IOPX_HASH_BLAKE2B && bcs_hash_type != IOPX_HASH_POSEIDON_STARKWARE && bcs_hash_type != IOPX_HASH_POSEIDON_HIGH_ALPHA)
            throw std::invalid_argument("bcs_hash_type unknown");
        if (bcs_hash_type != IOPX_HASH_BLAKE2B && gf64) throw std::invalid_argument("gf64 proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
        if (bcs_hash_type != IOPX_HASH_BLAKE2B && gfx)
            throw std::invalid_argument(std::string(gfx_name()) + " proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
        if (bcs_hash_type != IOPX_HASH_BLAKE2B && !bn128) throw std::invalid_argument("Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
        if (bn128 && comm) throw std::invalid_argument("alt_bn128 Fr has no distributed prover: pass no communicator");
        if (gf64 && comm) throw std::invalid_argument("gf64 has no distributed prover: pass no communicator");
        if (gfx && comm) throw std::invalid_argument(std::string(gfx_name()) + " has no distributed prover: pass no communicator");
        require_supported_security(security_parameter);
        const dist::scope bound(comm);
        const aurora_snark_parameters<F> params(cs.num_constraints(), cs.num_variables(), cs.num_inputs(), security_parameter, RS_extra_dimensions,
                                                FRI_localization_parameter);
        if (bn128 && params.codeword_domain_dim_ > 28)
            throw std::invalid_argument("codeword domain dimension " + std::to_string(params.codeword_domain_dim_) + ": alt_bn128 Fr has subgroups of order up to 2^28");
        if (gf64 && params.codeword_domain_dim_ > IOPX_GF64_MAX_DOMAIN_DIM)            // before any device work
            throw std::invalid_argument("codeword domain dimension " + std::to_string(params.codeword_domain_dim_) + ": the gf64 transforms take domains of dimension up to " +
                                        std::to_string(IOPX_GF64_MAX_DOMAIN_DIM));
        if (gfx && params.codeword_domain_dim_ > IOPX_GFX_MAX_DOMAIN_DIM)              // before any device work
            throw std::invalid_argument("codeword domain dimension " + std::to_string(params.codeword_domain_dim_) + ": the " + gfx_name() +
                                        " transforms take domains of dimension up to " + std::to_string(IOPX_GFX_MAX_DOMAIN_DIM));
        if constexpr (bn128) {
            if (bcs_hash_type != IOPX_HASH_BLAKE2B) return aurora_snark_prover_serialized<F, poseidon>(cs, primary, auxiliary, params, &d_assignment, poseidon(bcs_hash_type));
        }
        return aurora_snark_prover_serialized<F>(cs, primary, auxiliary, params, &d_assignment);
    }
};

template<typename F>
InstanceBase *make_from_csr(const iopx_r1cs *r, const uint64_t *assignment)
{
    for (int q = 0; q < 3; ++q) {                                // the offsets are trusted by every later matrix kernel: check them here
        const uint64_t *rp = r->row_ptr[q];
        if (rp[0] != 0) throw std::invalid_argument("iopx_aurora_instance_create: row_ptr must start at 0");
        for (size_t i = 0; i < r->num_constraints; ++i)
            if (rp[i + 1] < rp[i]) throw std::invalid_argument("iopx_aurora_instance_create: row_ptr must be non-decreasing");
    }
    std::unique_ptr<Instance<F>> holder(new Instance<F>());      // released to the caller only when fully built
    Instance<F> *inst = holder.get();
    inst->cs.primary_input_size_ = r->num_inputs;
    inst->cs.auxiliary_input_size_ = r->num_variables - r->num_inputs;
    sparse_matrix<F> *M[3] = { &inst->cs.A, &inst->cs.B, &inst->cs.C };
    for (int q = 0; q < 3; ++q) {
        M[q]->rows = r->num_constraints;
        M[q]->row_ptr.assign(r->row_ptr[q], r->row_ptr[q] + r->num_constraints + 1);
        const size_t nnz = (size_t)r->row_ptr[q][r->num_constraints];
        M[q]->col.assign(r->col[q], r->col[q] + nnz);
        M[q]->coeff.resize(nnz);
        if (nnz) std::memcpy((void *)M[q]->coeff.data(), r->coeff[q], nnz * sizeof(F));
        for (uint32_t c : M[q]->col) if (c > r->num_variables) throw std::invalid_argument("iopx_aurora_instance_create: column index exceeds the number of variables");
    }
    inst->primary.resize(r->num_inputs);
    inst->auxiliary.resize(r->num_variables - r->num_inputs);
    if (r->num_inputs) std::memcpy((void *)inst->primary.data(), assignment, r->num_inputs * sizeof(F));
    if (r->num_variables > r->num_inputs)
        std::memcpy((void *)inst->auxiliary.data(), assignment + sizeof(F) / 8 * r->num_inputs, (r->num_variables - r->num_inputs) * sizeof(F));
    inst->finish();
    return holder.release();
}

template<typename F>
InstanceBase *make_example(size_t num_constraints, size_t num_inputs, size_t num_variables, uint64_t seed)
{
    std::unique_ptr<Instance<F>> holder(new Instance<F>());
    Instance<F> *inst = holder.get();
    r1cs_example<F> ex = generate_r1cs_example<F>(num_constraints, num_inputs, num_variables, seed);
    inst->cs = std::move(ex.constraint_system);
    inst->primary = std::move(ex.primary_input);
    inst->auxiliary = std::move(ex.auxiliary_input);
    inst->finish();
    return holder.release();
}

template<typename Fn>
int guarded(Fn fn)
{
    try {
        fn();
        return IOPX_OK;
    } catch (const std::invalid_argument &e) {
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "%s", e.what());
    } catch (const std::logic_error &e) {
        return iopx::fail(IOPX_ERR_LOGIC, "%s", e.what());
    } catch (const std::bad_alloc &) {
        return iopx::fail(IOPX_ERR_RUNTIME, "out of host memory");
    } catch (const std::exception &e) {
        // a failure inside a nested C-ABI call has already recorded its message; keep the outer wording when it is more specific
        return iopx::fail(IOPX_ERR_RUNTIME, "%s", e.what());
    }
}

template<typename F, typename HashPolicy>
std::string fri_prove(iopx_comm *comm, const uint64_t *d_coeffs, size_t n_coeffs, const FRI_snark_parameters &params, const HashPolicy &hash)
{
    const dist::scope bound(comm);
    device_vector<F> coeffs(n_coeffs);
    if (n_coeffs) check(iopx_memcpy_d2d(coeffs.data(), d_coeffs, n_coeffs * sizeof(F)));
    return FRI_snark_prover_serialized<F, HashPolicy>(coeffs, params, hash);
}

int fri_entry(int field, int bcs_hash_type, iopx_comm *comm, const uint64_t *d_poly_coeffs, size_t n_coeffs, size_t codeword_domain_dim, size_t RS_extra_dimensions,
              size_t FRI_localization_parameter, size_t num_interactive_repetitions, size_t num_query_repetitions, uint8_t **transcript, size_t *transcript_bytes)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!transcript || !transcript_bytes || (n_coeffs && !d_poly_coeffs)) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    if (field == IOPX_FIELD_GF64 && codeword_domain_dim > IOPX_GF64_MAX_DOMAIN_DIM)
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "codeword domain dimension %zu: the gf64 transforms take domains of dimension up to %d", codeword_domain_dim, IOPX_GF64_MAX_DOMAIN_DIM);
    if (codeword_domain_dim > 40) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "codeword domain dimension %zu too large", codeword_domain_dim);
    if (field == IOPX_FIELD_GF64 && comm) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf64 has no distributed prover: pass no communicator");
    if (field == IOPX_FIELD_GF64 && bcs_hash_type != IOPX_HASH_BLAKE2B && (bcs_hash_type == IOPX_HASH_POSEIDON_STARKWARE || bcs_hash_type == IOPX_HASH_POSEIDON_HIGH_ALPHA))
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf64 proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
    if (field == IOPX_FIELD_GF128 && comm) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf128 has no distributed prover: pass no communicator");
    if (field == IOPX_FIELD_GF256 && comm) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf256 has no distributed prover: pass no communicator");
    if (field == IOPX_FIELD_GF128 && bcs_hash_type != IOPX_HASH_BLAKE2B && (bcs_hash_type == IOPX_HASH_POSEIDON_STARKWARE || bcs_hash_type == IOPX_HASH_POSEIDON_HIGH_ALPHA))
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf128 proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
    if (field == IOPX_FIELD_GF256 && bcs_hash_type != IOPX_HASH_BLAKE2B && (bcs_hash_type == IOPX_HASH_POSEIDON_STARKWARE || bcs_hash_type == IOPX_HASH_POSEIDON_HIGH_ALPHA))
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "gf256 proves with BLAKE2b: Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
    if (field == IOPX_FIELD_ALT_BN128_FR && codeword_domain_dim > 28)
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "codeword domain dimension %zu: alt_bn128 Fr has subgroups of order up to 2^28", codeword_domain_dim);
    if (field == IOPX_FIELD_ALT_BN128_FR && comm) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "alt_bn128 Fr has no distributed prover: pass no communicator");
    if (bcs_hash_type != IOPX_HASH_BLAKE2B && bcs_hash_type != IOPX_HASH_POSEIDON_STARKWARE && bcs_hash_type != IOPX_HASH_POSEIDON_HIGH_ALPHA)
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "bcs_hash_type unknown");
    if (bcs_hash_type != IOPX_HASH_BLAKE2B && field != IOPX_FIELD_ALT_BN128_FR && (field == IOPX_FIELD_GF192 || field == IOPX_FIELD_EDWARDS_FR))
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "Poseidon is wired for alt_bn128 Fr only (hash_enum.tcc:12-24)");
    return guarded([&] {
        const FRI_snark_parameters params(codeword_domain_dim, RS_extra_dimensions, FRI_localization_parameter, num_interactive_repetitions, num_query_repetitions);
        std::string t;
        if (field == IOPX_FIELD_GF192) t = fri_prove<gf192_element>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_EDWARDS_FR) t = fri_prove<edwards_Fr_element>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_GF64) t = fri_prove<libiop_amd::gf64>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_GF128) t = fri_prove<libiop_amd::gf128>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_GF256) t = fri_prove<libiop_amd::gf256>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_ALT_BN128_FR && bcs_hash_type == IOPX_HASH_BLAKE2B) t = fri_prove<alt_bn128_Fr_element>(comm, d_poly_coeffs, n_coeffs, params, blake2b());
        else if (field == IOPX_FIELD_ALT_BN128_FR) t = fri_prove<alt_bn128_Fr_element>(comm, d_poly_coeffs, n_coeffs, params, poseidon(bcs_hash_type));
        else throw std::invalid_argument("unknown field");
        uint8_t *buf = static_cast<uint8_t *>(std::malloc(t.size() ? t.size() : 1));
        if (!buf) throw std::bad_alloc();
        std::memcpy(buf, t.data(), t.size());
        *transcript = buf;
        *transcript_bytes = t.size();
    });
}

} // namespace

extern "C" {

int iopx_aurora_instance_create(const iopx_r1cs *r1cs, const uint64_t *assignment, int field, iopx_aurora_instance **out)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!r1cs || !assignment || !out) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    for (int q = 0; q < 3; ++q) if (!r1cs->row_ptr[q] || (!r1cs->col[q] && r1cs->row_ptr[q][r1cs->num_constraints]) || (!r1cs->coeff[q] && r1cs->row_ptr[q][r1cs->num_constraints]))
        return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null matrix array");
    if (r1cs->num_inputs > r1cs->num_variables) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "Number of inputs can't exceed number of variables.");
    return guarded([&] {
        if (field == IOPX_FIELD_GF192) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<gf192_element>(r1cs, assignment));
        else if (field == IOPX_FIELD_EDWARDS_FR) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<edwards_Fr_element>(r1cs, assignment));
        else if (field == IOPX_FIELD_ALT_BN128_FR) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<alt_bn128_Fr_element>(r1cs, assignment));
        else if (field == IOPX_FIELD_GF64) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<libiop_amd::gf64>(r1cs, assignment));
        else if (field == IOPX_FIELD_GF128) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<libiop_amd::gf128>(r1cs, assignment));
        else if (field == IOPX_FIELD_GF256) *out = reinterpret_cast<iopx_aurora_instance *>(make_from_csr<libiop_amd::gf256>(r1cs, assignment));
        else throw std::invalid_argument("unknown field");
    });
}

int iopx_aurora_example_instance_create(int field, size_t num_constraints, size_t num_inputs, size_t num_variables, uint64_t seed, iopx_aurora_instance **out)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!out) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return guarded([&] {
        if (field == IOPX_FIELD_GF192) *out = reinterpret_cast<iopx_aurora_instance *>(make_example<gf192_element>(num_constraints, num_inputs, num_variables, seed));
        else if (field == IOPX_FIELD_EDWARDS_FR) *out = reinterpret_cast<iopx_aurora_instance *>(make_example<edwards_Fr_element>(num_constraints, num_inputs, num_variables, seed));
        else if (field == IOPX_FIELD_ALT_BN128_FR) *out = reinterpret_cast<iopx_aurora_instance *>(make_example<alt_bn128_Fr_element>(num_constraints, num_inputs, num_variables, seed));
        else if (field == IOPX_FIELD_GF64) *out = reinterpret_cast<iopx_aurora_instance *>(make_example<libiop_amd::gf64>(num_constraints, num_inputs, num_variables, seed));
        // gf128, gf256: the synthetic instance is not generated over them (callers pass CSR matrices to iopx_aurora_instance_create); the wording dates from
        // before their protocol-layer kernels and is pinned by tests
        else if (field == IOPX_FIELD_GF128) throw std::invalid_argument("iopx_aurora_example_instance_create: only the FRI-only SNARK is built over gf128 (no protocol-layer kernels)");
        else if (field == IOPX_FIELD_GF256) throw std::invalid_argument("iopx_aurora_example_instance_create: only the FRI-only SNARK is built over gf256 (no protocol-layer kernels)");
        else throw std::invalid_argument("unknown field");
    });
}

static int prove_entry(iopx_aurora_instance *instance, iopx_comm *comm, bool fractal, size_t security_parameter, size_t RS_extra_dimensions,
                       size_t FRI_localization_parameter, uint8_t **transcript, size_t *transcript_bytes, int bcs_hash_type = IOPX_HASH_BLAKE2B)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!instance || !transcript || !transcript_bytes) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return guarded([&] {
        InstanceBase *inst = reinterpret_cast<InstanceBase *>(instance);
        const std::string t = fractal ? inst->fractal_prove(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter)
                                      : inst->prove(comm, bcs_hash_type, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        uint8_t *buf = static_cast<uint8_t *>(std::malloc(t.size() ? t.size() : 1));
        if (!buf) throw std::bad_alloc();
        std::memcpy(buf, t.data(), t.size());
        *transcript = buf;
        *transcript_bytes = t.size();
    });
}

static int index_entry(iopx_aurora_instance *instance, iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter,
                       uint8_t *index_roots, size_t root_capacity, size_t *num_roots)
{
    int rc = iopx::ensure_device();
    if (rc != IOPX_OK) return rc;
    if (!instance || !num_roots) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "null argument");
    return guarded([&] {
        const std::vector<std::string> roots = reinterpret_cast<InstanceBase *>(instance)->fractal_index(comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter);
        *num_roots = roots.size();
        if (index_roots) {
            if (root_capacity < roots.size()) throw std::invalid_argument("iopx_fractal_index: root buffer too small");
            for (size_t i = 0; i < roots.size(); ++i) std::memcpy(index_roots + 32 * i, roots[i].data(), 32);
        }
    });
}

// Everything a first proof would build and later ones find: the device pool at the size one proof needs (the largest single cost: the driver maps
// about 10 GB), the transforms' plans and twist / twiddle tables for every domain of this parameter set, the per-domain tables of the virtual oracles,
// the lincheck's transposed matrices (per instance), pinned staging.  They are keyed by what the proof's control flow asks for, so the way to build
// exactly them is to run that control flow once: a proof of the instance's own assignment, discarded.  protocol 1 (Fractal) needs the index.
int iopx_aurora_instance_warm(iopx_aurora_instance *instance, int protocol, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter)
{
    if (protocol != 0 && protocol != 1) return iopx::fail(IOPX_ERR_INVALID_ARGUMENT, "iopx_aurora_instance_warm: protocol %d (0: Aurora, 1: Fractal)", protocol);
    uint8_t *t = nullptr;
    size_t n = 0;
    const int rc = prove_entry(instance, nullptr, protocol == 1, security_parameter, RS_extra_dimensions, FRI_localization_parameter, &t, &n);
    std::free(t);
    return rc;
}

int iopx_aurora_prove(iopx_aurora_instance *instance, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter,
                      uint8_t **transcript, size_t *transcript_bytes)
{
    return prove_entry(instance, nullptr, false, security_parameter, RS_extra_dimensions, FRI_localization_parameter, transcript, transcript_bytes);
}

int iopx_aurora_prove_hashed(iopx_aurora_instance *instance, int bcs_hash_type, size_t security_parameter, size_t RS_extra_dimensions,
                             size_t FRI_localization_parameter, uint8_t **transcript, size_t *transcript_bytes)
{
    return prove_entry(instance, nullptr, false, security_parameter, RS_extra_dimensions, FRI_localization_parameter, transcript, transcript_bytes, bcs_hash_type);
}

int iopx_aurora_prove_dist(iopx_aurora_instance *instance, iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions,
                           size_t FRI_localization_parameter, uint8_t **transcript, size_t *transcript_bytes)
{
    return prove_entry(instance, comm, false, security_parameter, RS_extra_dimensions, FRI_localization_parameter, transcript, transcript_bytes);
}

int iopx_fractal_index(iopx_aurora_instance *instance, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter,
                       uint8_t *index_roots, size_t root_capacity, size_t *num_roots)
{
    return index_entry(instance, nullptr, security_parameter, RS_extra_dimensions, FRI_localization_parameter, index_roots, root_capacity, num_roots);
}

int iopx_fractal_index_dist(iopx_aurora_instance *instance, iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions,
                            size_t FRI_localization_parameter, uint8_t *index_roots, size_t root_capacity, size_t *num_roots)
{
    return index_entry(instance, comm, security_parameter, RS_extra_dimensions, FRI_localization_parameter, index_roots, root_capacity, num_roots);
}

int iopx_fractal_prove(iopx_aurora_instance *instance, size_t security_parameter, size_t RS_extra_dimensions, size_t FRI_localization_parameter,
                       uint8_t **transcript, size_t *transcript_bytes)
{
    return prove_entry(instance, nullptr, true, security_parameter, RS_extra_dimensions, FRI_localization_parameter, transcript, transcript_bytes);
}

int iopx_fractal_prove_dist(iopx_aurora_instance *instance, iopx_comm *comm, size_t security_parameter, size_t RS_extra_dimensions,
                            size_t FRI_localization_parameter, uint8_t **transcript, size_t *transcript_bytes)
{
    return prove_entry(instance, comm, true, security_parameter, RS_extra_dimensions, FRI_localization_parameter, transcript, transcript_bytes);
}

int iopx_fri_snark_prove_dist(int field, iopx_comm *comm, const uint64_t *d_poly_coeffs, size_t n_coeffs, size_t codeword_domain_dim, size_t RS_extra_dimensions,
                              size_t FRI_localization_parameter, size_t num_interactive_repetitions, size_t num_query_repetitions, uint8_t **transcript,
                              size_t *transcript_bytes)
{
    return fri_entry(field, IOPX_HASH_BLAKE2B, comm, d_poly_coeffs, n_coeffs, codeword_domain_dim, RS_extra_dimensions, FRI_localization_parameter,
                     num_interactive_repetitions, num_query_repetitions, transcript, transcript_bytes);
}

int iopx_fri_snark_prove_hashed(int field, int bcs_hash_type, const uint64_t *d_poly_coeffs, size_t n_coeffs, size_t codeword_domain_dim, size_t RS_extra_dimensions,
                                size_t FRI_localization_parameter, size_t num_interactive_repetitions, size_t num_query_repetitions, uint8_t **transcript,
                                size_t *transcript_bytes)
{
    return fri_entry(field, bcs_hash_type, nullptr, d_poly_coeffs, n_coeffs, codeword_domain_dim, RS_extra_dimensions, FRI_localization_parameter,
                     num_interactive_repetitions, num_query_repetitions, transcript, transcript_bytes);
}

int iopx_fri_snark_prove(int field, const uint64_t *d_poly_coeffs, size_t n_coeffs, size_t codeword_domain_dim, size_t RS_extra_dimensions,
                         size_t FRI_localization_parameter, size_t num_interactive_repetitions, size_t num_query_repetitions, uint8_t **transcript,
                         size_t *transcript_bytes)
{
    return iopx_fri_snark_prove_dist(field, nullptr, d_poly_coeffs, n_coeffs, codeword_domain_dim, RS_extra_dimensions, FRI_localization_parameter,
                                     num_interactive_repetitions, num_query_repetitions, transcript, transcript_bytes);
}

int iopx_aurora_instance_free(iopx_aurora_instance *instance)
{
    delete reinterpret_cast<InstanceBase *>(instance);
    return IOPX_OK;
}

int iopx_host_free(void *p)
{
    std::free(p);
    return IOPX_OK;
}

} // extern "C"
