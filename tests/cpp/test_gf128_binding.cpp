// The C++ seam over a 16-byte binary field: additive_FFT<gf128> / additive_IFFT<gf128>, the *_over_field_subset dispatch and the additive
// evaluate_next_f_i_over_entire_domain of libiop_amd/cpp/libiop_amd.hpp with the plain gf128 type of cpp/fields.hpp.  FFT then IFFT must
// round-trip, the dispatchers must agree with the templates, and the fold through the template must equal the C entry; the outputs are
// written for tests/test_gf128_binding.py to compare with the oracle.
//   usage: test_gf128_binding DIR      (reads DIR/in_*.bin, writes DIR/out_*.bin)
#include "libiop_amd/cpp/libiop_amd.hpp"
#include "libiop_amd/cpp/fields.hpp"
#include <cstdio>
#include <string>

typedef libiop_amd::gf128 F;
static_assert(sizeof(F) == 16, "gf128 is two 64-bit words");

static std::vector<F> read_elems(const std::string &path)
{
    std::vector<F> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot open %s\n", path.c_str()); std::exit(3); }
    F x;
    while (std::fread(x.w, 16, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

static void write_elems(const std::string &path, const std::vector<F> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    for (const F &x : v) std::fwrite(x.w, 16, 1, f);
    std::fclose(f);
}

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char **argv)
{
    using namespace libiop_amd;
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    if (iopx_init(0) != IOPX_OK) { std::printf("no device: %s\n", iopx_last_error()); return 2; }
    const std::vector<F> sc = read_elems(dir + "/in_scalars.bin");     // domain shift, fold x, then 7 basis vectors of a non-standard domain and its shift
    REQUIRE(sc.size() == 10);
    {   // 100 coefficients onto the shifted standard subspace of dimension 9, and back
        const std::vector<F> coeffs = read_elems(dir + "/in_fft.bin");
        const field_subset<F> D(512, sc[0]);
        const std::vector<F> evals = additive_FFT<F>(coeffs, D.subspace());
        REQUIRE(evals.size() == 512);
        REQUIRE(evals == FFT_over_field_subset<F>(coeffs, D));
        std::vector<F> padded = coeffs; padded.resize(512, F(0));
        REQUIRE(additive_IFFT<F>(evals, D.subspace()) == padded);
        REQUIRE(IFFT_over_field_subset<F>(evals, D) == padded);
        padded.resize(128);
        REQUIRE(IFFT_of_known_degree_over_field_subset<F>(evals, coeffs.size(), D) == padded);
        write_elems(dir + "/out_fft.bin", evals);
    }
    {   // a non-standard basis: round trip and fold with cosets of 4; the template against the C entry
        const std::vector<F> basis(sc.begin() + 2, sc.begin() + 9);
        const field_subset<F> D(affine_subspace<F>(basis, sc[9]));
        const auto f = std::make_shared<std::vector<F>>(read_elems(dir + "/in_fold.bin"));
        REQUIRE(f->size() == 128);
        REQUIRE(additive_FFT<F>(additive_IFFT<F>(*f, D.subspace()), D.subspace()) == *f);
        const auto next = evaluate_next_f_i_over_entire_domain<F>(f, D, 4, sc[1]);
        REQUIRE(*next == *additive_evaluate_next_f_i_over_entire_domain<F>(f, D, 4, sc[1]));
        std::vector<F> direct(32);
        const F shift = D.shift();
        check(iopx_fri_fold_add_gf128(f->data()->w, basis.data()->w, 7, shift.w, 4, sc[1].w, direct.data()->w));
        REQUIRE(*next == direct);
        write_elems(dir + "/out_fold.bin", *next);
    }
    {   // no multiplicative coset exists over a binary field
        bool refused = false;
        try { multiplicative_coset<F> c(8, F(1)); } catch (const std::invalid_argument &) { refused = true; }
        REQUIRE(refused);
    }
    std::printf("gf128 binding ok\n");
    return 0;
}
