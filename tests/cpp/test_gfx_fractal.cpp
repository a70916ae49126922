// The C++ seam of what the Fractal prover needs over the 8-, 16- and 32-byte binary fields: dev::div, dev::domain_offsets, dev::vanishing_evals and the
// table slots rational_combine and rational_sumcheck_constraint of libiop_amd/cpp/field_ops.hpp instantiated for gf64, gf128 and gf256 of
// cpp/fields.hpp and held to the host's products, and fractal_snark_indexer / fractal_snark_prover<gf64> under IOPX_GFX_FRACTAL=1 on a constraint
// system built row by row.  The index roots and the transcript's bytes are written for tests/test_gfx_fractal_binding.py, which compares them with
// the C ABI's and the oracle's.
//   usage: test_gfx_fractal DIR      (reads DIR/in_system.bin as tests/cpp/test_gf64_aurora.cpp does, writes DIR/out_roots.bin and DIR/out_transcript.bin)
#include "libiop_amd/cpp/aurora.hpp"
#include "libiop_amd/cpp/fractal.hpp"
#include "libiop_amd/cpp/fields.hpp"
#include <cstdio>
#include <string>

using namespace libiop_amd;

#define REQUIRE(c) do { if (!(c)) { std::printf("%s: %s failed\n", name, #c); return false; } } while (0)

template<typename T>
static bool operators(const char *name)
{
    typedef field_host<T> H;
    const std::size_t m = 5, n = (std::size_t)1 << m, k = 2;
    const field_subset<T> D(n, T((uint64_t)1 << 20)), K((std::size_t)1 << k);
    std::vector<T> x(n);
    for (std::size_t j = 0; j < n; ++j) x[j] = T(((uint64_t)1 << 20) ^ j);          // the standard basis: element j is shift + j
    const T point(0x1234567), constant(0x77), mu(0xABCDEF);
    const std::vector<T> off = dev::domain_offsets<T>(D, point).to_host();
    for (std::size_t j = 0; j < n; ++j) REQUIRE(off[j] == point + x[j]);
    std::vector<T> Z(n);                                                             // Z_K(x) = prod over K of (x + s)
    for (std::size_t j = 0; j < n; ++j) {
        Z[j] = H::one();
        for (uint64_t s = 0; s < ((uint64_t)1 << k); ++s) Z[j] = H::mul(Z[j], x[j] + T(s));
        REQUIRE(H::vanishing_eval(K, x[j]) == Z[j]);
    }
    const std::vector<T> ev = dev::vanishing_evals<T>(K, D, constant).to_host();
    for (std::size_t j = 0; j < n; ++j) REQUIRE(ev[j] == constant + Z[j]);
    const device_vector<T> d_x = dev::domain_elements<T>(D), d_num = dev::domain_offsets<T>(D, point);
    const std::vector<T> q = dev::div<T>(&d_num, d_x).to_host(), xinv = dev::div<T>(nullptr, d_x).to_host();
    for (std::size_t j = 0; j < n; ++j) REQUIRE(H::mul(q[j], x[j]) == off[j] && H::mul(xinv[j], x[j]) == H::one());
    // two rationals N_i / D_i with N = (x, off), D = (off, x): N = c0 x x + c1 off off, D = off x
    const std::vector<T> c = { T(5), T(9) };
    const void *Ns[2] = { d_x.data(), d_num.data() }, *Ds[2] = { d_num.data(), d_x.data() };
    device_vector<T> oN(n), oD(n);
    check(field_entry<T>(&ops::vector_ops::rational_combine, "rational_combine")(Ns, Ds, 2, detail::words(c.data()), n, oN.words(), oD.words()));
    const std::vector<T> hN = oN.to_host(), hD = oD.to_host();
    for (std::size_t j = 0; j < n; ++j) {
        REQUIRE(hD[j] == H::mul(off[j], x[j]));
        REQUIRE(hN[j] == H::mul(H::mul(c[0], x[j]), x[j]) + H::mul(H::mul(c[1], off[j]), off[j]));
    }
    // the constraint oracle with p = x, N = off, D = the combined denominator: out Z_K = D (p + eps^-1 mu x^(|K| - 1)) + N, eps = 1 * 2 * 3
    const device_vector<T> d_xinv = dev::div<T>(nullptr, d_x);
    device_vector<T> out(n);
    const T kshift = H::zero();
    check(ops::rational_sumcheck_constraint<field_of<T>>(dev::domain_words<T>(D), d_x.words(), d_num.words(), oD.words(), d_xinv.words(), k, detail::words(&kshift),
                                                         detail::words(&mu), out.words()));
    const std::vector<T> got = out.to_host();
    const T cc = H::mul(H::inverse(H::mul(T(2), T(3))), mu);
    for (std::size_t j = 0; j < n; ++j) {
        const T x3 = H::mul(H::mul(x[j], x[j]), x[j]);                               // x^(|K| - 1)
        REQUIRE(H::mul(got[j], Z[j]) == H::mul(hD[j], x[j] + H::mul(cc, x3)) + off[j]);
    }
    return true;
}

int main(int argc, char **argv)
{
    typedef libiop_amd::gf64 F;
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    if (iopx_init(0) != IOPX_OK) { std::printf("no device: %s\n", iopx_last_error()); return 2; }
    std::vector<uint64_t> w;
    {
        FILE *f = std::fopen((dir + "/in_system.bin").c_str(), "rb");
        if (!f) { std::printf("cannot open the system\n"); return 3; }
        uint64_t x;
        while (std::fread(&x, 8, 1, f) == 1) w.push_back(x);
        std::fclose(f);
    }
    std::size_t at = 0;
    auto next = [&]() -> uint64_t { if (at >= w.size()) { std::printf("the system file is short\n"); std::exit(3); } return w[at++]; };
    const std::size_t n = next(), vars = next(), inputs = next(), rs_extra = next(), loc = next();
    std::vector<linear_combination<F>> rows[3];
    for (int q = 0; q < 3; ++q) {
        std::vector<uint64_t> row_ptr(n + 1);
        for (auto &v : row_ptr) v = next();
        std::vector<uint64_t> col(row_ptr[n]), coeff(row_ptr[n]);
        for (auto &v : col) v = next();
        for (auto &v : coeff) v = next();
        rows[q].resize(n);
        for (std::size_t i = 0; i < n; ++i)
            for (uint64_t t = row_ptr[i]; t < row_ptr[i + 1]; ++t) rows[q][i].push_back(linear_term<F>{ (std::size_t)col[t], F(coeff[t]) });
    }
    r1cs_constraint_system<F> cs;
    cs.primary_input_size_ = inputs;
    cs.auxiliary_input_size_ = vars - inputs;
    for (std::size_t i = 0; i < n; ++i) cs.add_constraint({ rows[0][i], rows[1][i], rows[2][i] });
    std::vector<F> primary, auxiliary;
    for (std::size_t i = 0; i < vars; ++i) (i < inputs ? primary : auxiliary).push_back(F(next()));
    if (at != w.size()) { std::printf("the system file is long\n"); return 3; }
    try {
        // with the option unset the host's Z_S stays refused over these fields; the device operators do not depend on it
        bool refused = false;
        try { (void)field_host<F>::vanishing_eval(field_subset<F>(8), F(3)); } catch (const std::invalid_argument &) { refused = true; }
        if (!refused) { std::printf("vanishing_eval over gf64 was not refused with the option unset\n"); return 1; }
        check(iopx_set_option("IOPX_GFX_FRACTAL", 1));
        if (!operators<libiop_amd::gf64>("gf64") || !operators<libiop_amd::gf128>("gf128") || !operators<libiop_amd::gf256>("gf256")) return 1;
        const fractal_snark_parameters<F> params(cs, 128, rs_extra, loc);
        if (params.holographic_lincheck_repetitions_ != 3 || params.num_output_LDT_instances_ != 3 || params.fri_interactive_repetitions_ != 3) {
            std::printf("unexpected repetition counts\n");
            return 1;
        }
        const auto index = fractal_snark_indexer<F>(cs, params);
        const std::string t = fractal_snark_prover<F>(index.first, cs, primary, auxiliary, params).serialize();
        if (t != fractal_snark_prover_serialized<F>(index.first, cs, primary, auxiliary, params)) { std::printf("the two provers' bytes differ\n"); return 1; }
        FILE *f = std::fopen((dir + "/out_roots.bin").c_str(), "wb");
        for (const std::string &r : index.second.index_MT_roots_) std::fwrite(r.data(), 1, r.size(), f);
        std::fclose(f);
        f = std::fopen((dir + "/out_transcript.bin").c_str(), "wb");
        std::fwrite(t.data(), 1, t.size(), f);
        std::fclose(f);
        check(iopx_clear_option("IOPX_GFX_FRACTAL"));
    } catch (const std::exception &e) {
        std::printf("failed: %s (%s)\n", e.what(), iopx_last_error());
        return 1;
    }
    std::printf("gfx fractal ok\n");
    return 0;
}
