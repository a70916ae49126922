// The alt_bn128 Fr stubs of INTEGRATION.md ("alt_bn128 Fr", blocks marked bn128:def), compiled verbatim by tests/test_bn128_binding.py
// (which writes them to bn128_stubs.inc) against the mirror classes of libiop_amd/cpp/libiop_amd.hpp, with libff::alt_bn128_Fr = the 32-byte
// stand-in of cpp/fields.hpp.  The program runs one FFT, fold and LDT combination case of tests/golden/bn128_tiny.json through the stubs
// and through the mirror's own dispatchers (FFT_over_field_subset, evaluate_next_f_i_over_entire_domain), requires the two to agree, and
// writes the stubs' outputs for the test to digest.
//   usage: test_bn128_binding DIR      (reads DIR/in_*.bin, writes DIR/out_*.bin)
#include "libiop_amd/cpp/libiop_amd.hpp"
#include "libiop_amd/cpp/fields.hpp"
#include <cstdio>
#include <string>

namespace libff { typedef libiop_amd::alt_bn128_Fr_element alt_bn128_Fr; }
namespace libiop {
using libiop_amd::multiplicative_coset; using libiop_amd::field_subset; using libiop_amd::multiplicative_coset_type;
// the reference's primary templates, declared with its signatures (fft.hpp:46-52, fri_aux.tcc:106-111)
template<typename FieldT> std::vector<FieldT> multiplicative_FFT(const std::vector<FieldT> &poly_coeffs, const multiplicative_coset<FieldT> &domain);
template<typename FieldT> std::vector<FieldT> multiplicative_IFFT(const std::vector<FieldT> &evals, const multiplicative_coset<FieldT> &domain);
template<typename FieldT> std::shared_ptr<std::vector<FieldT>> multiplicative_evaluate_next_f_i_over_entire_domain(
    const std::shared_ptr<std::vector<FieldT>> &f_i_evals, const field_subset<FieldT> &f_i_domain, const size_t coset_size, const FieldT x_i);
// the members of combined_LDT_virtual_oracle (ldt_reducer_aux.hpp) that evaluated_contents reads, public here
template<typename FieldT>
class combined_LDT_virtual_oracle {
public:
    field_subset<FieldT> codeword_domain_;
    std::vector<std::size_t> input_oracle_degrees_;
    std::vector<FieldT> coefficients_;
    std::shared_ptr<std::vector<FieldT>> evaluated_contents(const std::vector<std::shared_ptr<std::vector<FieldT>>> &constituent_oracle_evaluations) const;
};
#include "bn128_stubs.inc"
}

typedef libff::alt_bn128_Fr F;

static std::vector<F> read_elems(const std::string &path)
{
    std::vector<F> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot open %s\n", path.c_str()); std::exit(3); }
    F x;
    while (std::fread(x.w, 8, 4, f) == 4) v.push_back(x);
    std::fclose(f);
    return v;
}

static void write_elems(const std::string &path, const std::vector<F> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    for (const F &x : v) std::fwrite(x.w, 8, 4, f);
    std::fclose(f);
}

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char **argv)
{
    using namespace libiop_amd;
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    if (iopx_init(0) != IOPX_OK) { std::printf("no device: %s\n", iopx_last_error()); return 2; }
    const std::vector<F> sc = read_elems(dir + "/in_scalars.bin");     // fft shift, fold shift, fold x, 6 LDT coefficients
    REQUIRE(sc.size() == 9);
    {   // FFT of 33 coefficients over shift * <g>, |<g>| = 64, and back
        const std::vector<F> coeffs = read_elems(dir + "/in_fft.bin");
        const field_subset<F> D(64, sc[0]);
        const std::vector<F> evals = libiop::multiplicative_FFT<F>(coeffs, D.coset());
        REQUIRE(evals == FFT_over_field_subset<F>(coeffs, D));
        std::vector<F> padded = coeffs; padded.resize(64, F(0));
        REQUIRE(libiop::multiplicative_IFFT<F>(evals, D.coset()) == padded);
        REQUIRE(IFFT_over_field_subset<F>(evals, D) == padded);
        REQUIRE(IFFT_of_known_degree_over_field_subset<F>(evals, coeffs.size(), D) == padded);
        write_elems(dir + "/out_fft.bin", evals);
    }
    {   // fold with cosets of 4 over shift * <g>, |<g>| = 64
        const auto f = std::make_shared<std::vector<F>>(read_elems(dir + "/in_fold.bin"));
        const field_subset<F> D(64, sc[1]);
        const auto next = libiop::multiplicative_evaluate_next_f_i_over_entire_domain<F>(f, D, 4, sc[2]);
        REQUIRE(*next == *evaluate_next_f_i_over_entire_domain<F>(f, D, 4, sc[2]));
        write_elems(dir + "/out_fold.bin", *next);
    }
    {   // LDT combination of three oracles of 32 points, degrees 32, 20, 7, over 5 * <g>
        const std::vector<F> all = read_elems(dir + "/in_ldt.bin");
        std::vector<std::shared_ptr<std::vector<F>>> oracles;
        for (int k = 0; k < 3; ++k) oracles.push_back(std::make_shared<std::vector<F>>(all.begin() + 32 * k, all.begin() + 32 * (k + 1)));
        libiop::combined_LDT_virtual_oracle<F> ldt;
        ldt.codeword_domain_ = field_subset<F>(32, F(5));
        ldt.input_oracle_degrees_ = { 32, 20, 7 };
        ldt.coefficients_ = { F(1) };
        ldt.coefficients_.insert(ldt.coefficients_.end(), sc.begin() + 3, sc.end());
        write_elems(dir + "/out_ldt.bin", *ldt.evaluated_contents(oracles));
    }
    std::printf("bn128 stubs ok\n");
    return 0;
}
