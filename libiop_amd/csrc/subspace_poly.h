// The subspace polynomial over a binary field, host only and portable C++.  H is a field's host element (gf64_host.h, gf128_host.h,
// gf256_host.h): zero, one, +=, *, squared.
#pragma once
#include <cstddef>
#include <vector>

namespace iopx {

// The subspace polynomial of span(basis[0..dim)): prod_{v in span} (X - v), a linearized polynomial (coeff[i] multiplies X^(2^i)), built
// factor by factor as Z <- Z(X) (Z(X) + Z(b)) (libiop/algebra/polynomials/vanishing_polynomial.tcc:373-395).
template<class H>
struct SubspacePolyX {
    std::vector<H> coeff;
    SubspacePolyX(const H *basis, size_t dim) : coeff(1, H::one())
    {
        for (size_t k = 0; k < dim; ++k) {
            const H zb = eval(basis[k]);
            std::vector<H> nxt(coeff.size() + 1, H::zero());
            for (size_t i = 0; i < coeff.size(); ++i) { nxt[i + 1] += coeff[i].squared(); nxt[i] += coeff[i] * zb; }
            coeff.swap(nxt);
        }
    }
    H eval(const H &x) const
    {
        H r = H::zero(), xp = x;
        for (size_t i = 0; i < coeff.size(); ++i) { r += coeff[i] * xp; xp = xp.squared(); }
        return r;
    }
};

} // namespace iopx
