"""Evaluation domains and the two field arms of the accelerated path, host side (O(log n) metadata only).

`Domain` mirrors the reference's tagged union field_subset<FieldT> (libiop/algebra/field_subset/field_subset.tcc:3-62,
130-237): an affine subspace of GF(2^192) (subspace.tcc) or a multiplicative coset of the 181-bit prime field
(subgroup.tcc).  `GF192` / `EdwardsFr` carry what differs between the arms — scalar arithmetic on Python ints for the
handful of host-side constants, the hashchain extractor (blake2b.tcc:162-257), and `entries`, the table that takes every device
operator of `DeviceOps` to the matching C-ABI entry point (FFT_over_field_subset and friends dispatch on the domain type the same way,
fft.tcc:407-475, fri_aux.tcc:5-34).  Citations are relative to the reference tree."""
import hashlib

import numpy as np

import libiop_amd as la
from . import host

ADDITIVE, MULTIPLICATIVE = "affine_subspace", "multiplicative_coset"


def _log2(n):
    return max(int(n) - 1, 0).bit_length()          # libff::log2 is the ceiling log


class Domain:
    """field_subset<FieldT>."""

    def __init__(self, field, kind, basis=None, shift=None, log_n=None):
        self.field, self.kind = field, kind
        if kind == ADDITIVE:
            self.basis = np.ascontiguousarray(basis, dtype=np.uint64).reshape(-1, field.words)
            self.shift = np.ascontiguousarray(shift, dtype=np.uint64).reshape(field.words)
            self.dim = self.basis.shape[0]
        else:
            self.dim = int(log_n)
            self.shift_int = int(shift) % field.P                        # canonical integer
            if self.shift_int == 0:
                raise ValueError("coset_shift was supplied as 0, it was likely intended to be 1")
            self.shift = field.from_int(self.shift_int)
            self.gen = field.subgroup_generator(self.dim)                # subgroup.tcc:55-59
        self.size = 1 << self.dim

    # ---- what the device entries take (DeviceOps passes these on as they are) ----
    def args(self):
        """This domain as the domain an entry runs over: (basis, shift) of a subspace, (dim, gen, shift) of a coset."""
        return (self.basis, self.shift) if self.additive else (self.dim, self.gen, self.shift)

    def sub_args(self):
        """This domain as an entry's second domain (input, summation, vanishing): (basis, shift) / (dim, shift)."""
        return (self.basis, self.shift) if self.additive else (self.dim, self.shift)

    # ---- field_subset.tcc ----
    @property
    def additive(self):
        return self.kind == ADDITIVE

    @property
    def domain_type(self):
        return la.DOMAIN_ADDITIVE if self.additive else la.DOMAIN_MULTIPLICATIVE

    def num_elements(self):
        return self.size

    def dimension(self):
        return self.dim

    def get_subset_of_order(self, order):
        """:217-237 — first log2(order) basis vectors, same shift / the default subgroup of that order, same shift."""
        d = _log2(order)
        if self.additive:
            return Domain(self.field, ADDITIVE, basis=self.basis[:d], shift=self.shift)
        return Domain(self.field, MULTIPLICATIVE, shift=self.shift_int, log_n=d)

    def element_outside_of_subset(self):
        """subspace.tcc:219-227 (standard basis): shift + FieldT(1 << dim); subgroup.tcc:311-315: shift * multiplicative_generator."""
        if self.additive:
            if not np.array_equal(self.basis, self.field.standard_basis(self.dim)):
                raise ValueError("subspace.element_outside_of_subset() is only supported for standard basis")
            out = self.shift.copy()
            out[self.dim // 64] ^= np.uint64(1) << np.uint64(self.dim % 64)
            return out
        return (self.shift_int * self.field.GENERATOR) % self.field.P

    def reindex_by_subset(self, reindex_subset_dim, index):
        """:130-142; subgroup.tcc:149-173."""
        if self.additive:
            return index
        order_s, g_over_s = 1 << reindex_subset_dim, 1 << (self.dim - reindex_subset_dim)
        if index < order_s:
            return index * g_over_s
        i = index - order_s
        return i + (i // (g_over_s - 1)) + 1

    def reindex_by_subset_array(self, reindex_subset_dim, count):
        """reindex_by_subset(dim, i) for i < count, vectorised."""
        idx = np.arange(count, dtype=np.int64)
        if self.additive:
            return idx
        order_s, g_over_s = 1 << reindex_subset_dim, 1 << (self.dim - reindex_subset_dim)
        i = idx - order_s
        return np.where(idx < order_s, idx * g_over_s, i + (i // max(g_over_s - 1, 1)) + 1)

    # coset index maps (subspace.tcc:73-91, subgroup.tcc:175-197)
    def coset_index(self, position, coset_size):
        return position // coset_size if self.additive else position % (self.size // coset_size)

    def intra_coset_index(self, position, coset_size):
        return position % coset_size if self.additive else position // (self.size // coset_size)

    def position_by_coset_indices(self, coset_index, intra_coset_index, coset_size):
        if self.additive:
            return coset_index * coset_size + intra_coset_index
        return coset_index + intra_coset_index * (self.size // coset_size)


class GF192:
    """libff::gf192, additive arm."""
    name, additive, elem_bytes, words, soundness_bits = "gf192", True, 24, 3, 192
    standard_basis = staticmethod(la.standard_basis)
    # DeviceOps operator (or optional slot) -> (Library method, its fixed keyword arguments)
    entries = {
        "FFT": ("additive_FFT_dev", {}),
        "IFFT": ("additive_IFFT_dev", {}),
        "LDE_batch": ("additive_LDE_batch_dev", {}),                    # optional: FFT_batch
        "IFFT_batch": ("additive_IFFT_batch_dev", {}),                  # optional: IFFT_batch, IFFT_batch_packed
        "reextend_batch": ("additive_reextend_batch_dev", {}),          # optional: reextend_packed, fused
        "fold": ("fri_fold_dev", {}),
        "ldt_combine": ("ldt_combine_dev", {}),
        "rowcheck": ("rowcheck_dev", {}),
        "fz": ("fz_dev", {}),
        "sumcheck_g": ("sumcheck_g_dev", {}),
        "lincheck": ("lincheck_dev", {}),
        "lincomb": ("lincomb_dev", {}),
        "lincomb_affine": ("lincomb_affine_dev", {}),
        "sub": ("field_add_dev", {}),
        "mul": ("gf192_mul_dev", {}),
        "inv": ("field_inv_dev", {}),
        "pow_table": ("pow_table_dev", {}),
        "spmv": ("spmv_dev", {}),
        "div": ("field_div_dev", {}),
        "domain_offsets": ("domain_offsets_dev", {}),
        "vanishing_evals": ("vanishing_evals_dev", {}),
        "rational_combine": ("rational_combine_dev", {}),
        "rational_sumcheck_constraint": ("rational_sumcheck_constraint_dev", {}),
        "poly_div_vanishing": ("poly_div_vanishing_dev", {}),
    }

    def domain(self, num_elements, shift=None):
        """field_subset(num_elements[, shift]) — field_subset.tcc:3-18,45-62."""
        d = _log2(num_elements)
        return Domain(self, ADDITIVE, basis=self.standard_basis(d), shift=np.zeros(3, dtype=np.uint64) if shift is None else shift)

    # host scalars: (3,) uint64 words
    def zero(self):
        return np.zeros(3, dtype=np.uint64)

    def mul(self, a, b):
        return host.gf_to_words(host.gf_mul(host.gf_from_words(a), host.gf_from_words(b)))

    def add(self, a, b):
        return np.bitwise_xor(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))

    def sub(self, a, b):
        return self.add(a, b)

    def neg(self, a):
        return np.asarray(a, dtype=np.uint64)

    def one(self):
        return np.array([1, 0, 0], dtype=np.uint64)

    def inv(self, a, lib):
        return lib.gf192_inverse_host(a)

    def vanishing_eval(self, domain, x, lib):
        """Z_S(x) for the affine subspace S (vanishing_polynomial::evaluation_at_point)."""
        return lib.gf192_vanishing_host(domain.basis, domain.shift, x)[0]

    def vanishing_derivative(self, domain, x, lib):
        """(DZ_S)(x): the linear coefficient (vanishing_polynomial.tcc:63-72)."""
        return lib.gf192_vanishing_host(domain.basis, domain.shift, x)[1]

    def element_in_domain(self, domain, x):
        v = host.gf_from_words(self.add(x, domain.shift))
        if not np.array_equal(domain.basis, self.standard_basis(domain.dim)):
            raise NotImplementedError("membership test for a non-standard basis")
        return v < (1 << domain.dim)

    def squeeze(self, hashchain, n):
        return hashchain.squeeze_gf192(n)

    def fri_domains(self, domain, localization, lib):
        """FRI_protocol::compute_domains, additive branch (fri_ldt.tcc:310-338), by the library's host-side helper."""
        chain = lib.fri_additive_domains(domain.basis, domain.shift, localization)
        return [domain] + [Domain(self, ADDITIVE, basis=b, shift=s) for b, s in chain[1:]]


class GF64:
    """libff::gf64 (x^64 + x^4 + x^3 + x + 1, one word), additive arm.  Host scalars are (1,) uint64 arrays; the handful of host-side
    products run on Python integers."""
    name, additive, elem_bytes, words, soundness_bits = "gf64", True, 8, 1, 64
    entries = {
        "FFT": ("additive_FFT_gf64_dev", {}),
        "IFFT": ("additive_IFFT_gf64_dev", {}),
        "LDE": ("additive_LDE_gf64_dev", {}),                           # optional: reextend_packed, one vector at a time
        "LDE_batch": ("additive_LDE_batch_dev", {"words": 1}),          # optional: FFT_batch
        "IFFT_batch": ("additive_IFFT_batch_dev", {"words": 1}),        # optional: IFFT_batch, IFFT_batch_packed
        "reextend_batch": ("additive_reextend_batch_dev", {"words": 1}),  # optional: reextend_packed, fused
        "fold": ("evaluate_next_f_i_over_entire_domain_gf64_dev", {}),
        "ldt_combine": ("ldt_combine_gf64_dev", {}),
        "rowcheck": ("rowcheck_dev", {"words": 1}),
        "fz": ("fz_dev", {"words": 1}),
        "sumcheck_g": ("sumcheck_g_dev", {"words": 1}),
        "lincheck": ("lincheck_dev", {"words": 1}),
        "lincomb": ("lincomb_dev", {"words": 1}),
        "lincomb_affine": ("lincomb_affine_dev", {"words": 1}),
        "sub": ("field_add_dev", {"words": 1}),
        "mul": ("gf64_mul_dev", {}),
        "inv": ("gf64_inv_dev", {}),
        "pow_table": ("pow_table_dev", {"words": 1}),
        "spmv": ("spmv_dev", {"words": 1}),
        "poly_div_vanishing": ("poly_div_vanishing_dev", {"words": 1}),
        # what Fractal calls beyond Aurora: the entries of include/libiop_amd_fractal.h
        "div": ("field_div_dev", {"words": 1}),
        "domain_offsets": ("domain_offsets_dev", {"words": 1}),
        "vanishing_evals": ("vanishing_evals_dev", {"words": 1}),
        "rational_combine": ("rational_combine_dev", {"words": 1}),
        "rational_sumcheck_constraint": ("rational_sumcheck_constraint_dev", {"words": 1}),
    }

    @staticmethod
    def standard_basis(m):
        """subspace.tcc:93-108 — basis element i is FieldT(1 << i)."""
        return (np.uint64(1) << np.arange(m, dtype=np.uint64)).reshape(m, 1)

    def domain(self, num_elements, shift=None):
        d = _log2(num_elements)
        return Domain(self, ADDITIVE, basis=self.standard_basis(d), shift=np.zeros(1, dtype=np.uint64) if shift is None else shift)

    @staticmethod
    def _int(a):
        return int(np.asarray(a, dtype=np.uint64).reshape(-1)[0])

    @staticmethod
    def _elem(v):
        return np.array([v], dtype=np.uint64)

    @staticmethod
    def _mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            b >>= 1
            a <<= 1
            if a >> 64:
                a ^= (1 << 64) | 0x1B
        return r

    def zero(self):
        return np.zeros(1, dtype=np.uint64)

    def one(self):
        return self._elem(1)

    def mul(self, a, b):
        return self._elem(self._mul(self._int(a), self._int(b)))

    def add(self, a, b):
        return np.bitwise_xor(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))

    def sub(self, a, b):
        return self.add(a, b)

    def neg(self, a):
        return np.asarray(a, dtype=np.uint64)

    def inv(self, a, lib):
        return lib.gf64_inverse_host(a)

    def _subspace_poly(self, domain):
        """coefficients c_i of prod_{v in span(basis)} (X - v) = sum_i c_i X^(2^i) (vanishing_polynomial.tcc:373-395)"""
        def ev(c, x):
            r = 0
            for ci in c:
                r ^= self._mul(ci, x)
                x = self._mul(x, x)
            return r
        c = [1]
        for b in domain.basis[:, 0]:
            zb = ev(c, int(b))
            nxt = [0] * (len(c) + 1)
            for i, ci in enumerate(c):
                nxt[i + 1] ^= self._mul(ci, ci)
                nxt[i] ^= self._mul(ci, zb)
            c = nxt
        return c, ev

    def vanishing_eval(self, domain, x, lib=None):
        """Z_S(x) for the affine subspace S: the subspace polynomial at x plus at the shift."""
        c, ev = self._subspace_poly(domain)
        return self._elem(ev(c, self._int(x)) ^ ev(c, self._int(domain.shift)))

    def vanishing_derivative(self, domain, x, lib=None):
        """(DZ_S)(x): the linear coefficient (vanishing_polynomial.tcc:63-72)."""
        return self._elem(self._subspace_poly(domain)[0][0])

    def element_in_domain(self, domain, x):
        if not np.array_equal(domain.basis, self.standard_basis(domain.dim)):
            raise NotImplementedError("membership test for a non-standard basis")
        return (self._int(x) ^ self._int(domain.shift)) < (1 << domain.dim)

    def squeeze(self, hashchain, n):
        """blake2b_FieldT_randomness_extractor for a binary field of 8 bytes (blake2b.tcc:162-185, 231-257): element i = keyed
        BLAKE2b(state || index, key = i, 8 bytes), the raw word."""
        hashchain.squeeze_index += 1
        msg = hashchain.state + hashchain.squeeze_index.to_bytes(8, "little")
        out = np.zeros((n, 1), dtype=np.uint64)
        for i in range(n):
            out[i, 0] = int.from_bytes(hashlib.blake2b(msg, digest_size=8, key=i.to_bytes(8, "little")).digest(), "little")
        return out

    def fri_domains(self, domain, localization, lib):
        """FRI_protocol::compute_domains, additive branch (fri_ldt.tcc:310-338), by the library's host-side helper."""
        chain = lib.fri_additive_domains_gf64(domain.basis, domain.shift, localization)
        return [domain] + [Domain(self, ADDITIVE, basis=b, shift=s) for b, s in chain[1:]]


class GF128(GF64):
    """libff::gf128 (x^128 + x^7 + x^2 + x + 1, two little-endian words), additive arm: the FRI-only SNARK and Aurora.  Host scalars are (2,) uint64
    arrays; the host-side products run on Python integers, as GF64's do."""
    name, additive, elem_bytes, words, soundness_bits = "gf128", True, 16, 2, 128
    # the transforms, the fold, the LDT combination and the vector helpers: the gf192 methods with two words per element
    entries = {
        "FFT": ("additive_FFT_dev", {"words": 2}),
        "IFFT": ("additive_IFFT_dev", {"words": 2}),
        "LDE": ("additive_LDE_dev", {"words": 2}),
        "LDE_batch": ("additive_LDE_batch_dev", {"words": 2}),          # optional: FFT_batch
        "IFFT_batch": ("additive_IFFT_batch_dev", {"words": 2}),        # optional: IFFT_batch, IFFT_batch_packed
        "reextend_batch": ("additive_reextend_batch_dev", {"words": 2}),  # optional: reextend_packed, fused
        "fold": ("fri_fold_dev", {"words": 2}),
        "ldt_combine": ("ldt_combine_dev", {"words": 2}),
        "sub": ("field_add_dev", {"words": 2}),
        "mul": ("gf192_mul_dev", {"words": 2}),
        "inv": ("field_inv_dev", {"words": 2}),
        # what Aurora calls beyond the FRI-only SNARK (GF128AuroraOps): the entries of csrc/gf128_ops.hip
        "rowcheck": ("rowcheck_dev", {"words": 2}),
        "fz": ("fz_dev", {"words": 2}),
        "sumcheck_g": ("sumcheck_g_dev", {"words": 2}),
        "lincheck": ("lincheck_dev", {"words": 2}),
        "lincomb": ("lincomb_dev", {"words": 2}),
        "lincomb_affine": ("lincomb_affine_dev", {"words": 2}),
        "pow_table": ("pow_table_dev", {"words": 2}),
        "spmv": ("spmv_dev", {"words": 2}),
        "poly_div_vanishing": ("poly_div_vanishing_dev", {"words": 2}),
        # what Fractal calls beyond Aurora: the entries of include/libiop_amd_fractal.h
        "div": ("field_div_dev", {"words": 2}),
        "domain_offsets": ("domain_offsets_dev", {"words": 2}),
        "vanishing_evals": ("vanishing_evals_dev", {"words": 2}),
        "rational_combine": ("rational_combine_dev", {"words": 2}),
        "rational_sumcheck_constraint": ("rational_sumcheck_constraint_dev", {"words": 2}),
    }
    _MASK = (1 << 64) - 1

    @staticmethod
    def standard_basis(m):
        """subspace.tcc:93-108 — basis element i is FieldT(1 << i)."""
        return np.array([[(1 << i) & GF128._MASK, (1 << i) >> 64] for i in range(m)], dtype=np.uint64).reshape(m, 2)

    def domain(self, num_elements, shift=None):
        d = _log2(num_elements)
        return Domain(self, ADDITIVE, basis=self.standard_basis(d), shift=np.zeros(2, dtype=np.uint64) if shift is None else shift)

    @staticmethod
    def _int(a):
        w = np.asarray(a, dtype=np.uint64).reshape(-1)
        return int(w[0]) | (int(w[1]) << 64)

    @staticmethod
    def _elem(v):
        return np.array([v & GF128._MASK, v >> 64], dtype=np.uint64)

    @staticmethod
    def _mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            b >>= 1
            a <<= 1
            if a >> 128:
                a ^= (1 << 128) | 0x87
        return r

    def zero(self):
        return np.zeros(2, dtype=np.uint64)

    def inv(self, a, lib):
        return lib.gf128_inverse_host(a)

    def _subspace_poly(self, domain):
        """coefficients c_i of prod_{v in span(basis)} (X - v) = sum_i c_i X^(2^i) (vanishing_polynomial.tcc:373-395)"""
        def ev(c, x):
            r = 0
            for ci in c:
                r ^= self._mul(ci, x)
                x = self._mul(x, x)
            return r
        c = [1]
        for b in domain.basis:
            zb = ev(c, self._int(b))
            nxt = [0] * (len(c) + 1)
            for i, ci in enumerate(c):
                nxt[i + 1] ^= self._mul(ci, ci)
                nxt[i] ^= self._mul(ci, zb)
            c = nxt
        return c, ev

    def squeeze(self, hashchain, n):
        """blake2b_FieldT_randomness_extractor for a binary field of 16 bytes (blake2b.tcc:162-185, 231-257): element i = keyed
        BLAKE2b(state || index, key = i, 16 bytes), the two raw words."""
        hashchain.squeeze_index += 1
        msg = hashchain.state + hashchain.squeeze_index.to_bytes(8, "little")
        out = np.zeros((n, 2), dtype=np.uint64)
        for i in range(n):
            out[i] = np.frombuffer(hashlib.blake2b(msg, digest_size=16, key=i.to_bytes(8, "little")).digest(), dtype="<u8")
        return out

    def fri_domains(self, domain, localization, lib):
        """FRI_protocol::compute_domains, additive branch (fri_ldt.tcc:310-338), by the library's host-side helper."""
        chain = lib.fri_additive_domains_gf128(domain.basis, domain.shift, localization)
        return [domain] + [Domain(self, ADDITIVE, basis=b, shift=s) for b, s in chain[1:]]


class GF256(GF128):
    """libff::gf256 (x^256 + x^10 + x^5 + x^2 + 1, four little-endian words), additive arm: the FRI-only SNARK and Aurora.  Host scalars are (4,) uint64
    arrays; the host-side products run on Python integers, as GF64's do."""
    name, additive, elem_bytes, words, soundness_bits = "gf256", True, 32, 4, 256
    # the transforms, the fold, the LDT combination and the vector helpers: the gf192 methods with four words per element
    entries = {
        "FFT": ("additive_FFT_dev", {"words": 4}),
        "IFFT": ("additive_IFFT_dev", {"words": 4}),
        "LDE": ("additive_LDE_dev", {"words": 4}),
        "LDE_batch": ("additive_LDE_batch_dev", {"words": 4}),          # optional: FFT_batch
        "IFFT_batch": ("additive_IFFT_batch_dev", {"words": 4}),        # optional: IFFT_batch, IFFT_batch_packed
        "reextend_batch": ("additive_reextend_batch_dev", {"words": 4}),  # optional: reextend_packed, fused
        "fold": ("fri_fold_dev", {"words": 4}),
        "ldt_combine": ("ldt_combine_dev", {"words": 4}),
        "sub": ("field_add_dev", {"words": 4}),
        "mul": ("gf192_mul_dev", {"words": 4}),
        "inv": ("field_inv_dev", {"words": 4}),
        # what Aurora calls beyond the FRI-only SNARK (GF256AuroraOps): the entries of csrc/gf256_ops.hip
        "rowcheck": ("rowcheck_dev", {"words": 4}),
        "fz": ("fz_dev", {"words": 4}),
        "sumcheck_g": ("sumcheck_g_dev", {"words": 4}),
        "lincheck": ("lincheck_dev", {"words": 4}),
        "lincomb": ("lincomb_dev", {"words": 4}),
        "lincomb_affine": ("lincomb_affine_dev", {"words": 4}),
        "pow_table": ("pow_table_dev", {"words": 4}),
        "spmv": ("spmv_dev", {"words": 4}),
        "poly_div_vanishing": ("poly_div_vanishing_dev", {"words": 4}),
        # what Fractal calls beyond Aurora: the entries of include/libiop_amd_fractal.h
        "div": ("field_div_dev", {"words": 4}),
        "domain_offsets": ("domain_offsets_dev", {"words": 4}),
        "vanishing_evals": ("vanishing_evals_dev", {"words": 4}),
        "rational_combine": ("rational_combine_dev", {"words": 4}),
        "rational_sumcheck_constraint": ("rational_sumcheck_constraint_dev", {"words": 4}),
    }

    @staticmethod
    def standard_basis(m):
        """subspace.tcc:93-108 — basis element i is FieldT(1 << i)."""
        return np.array([GF256._elem(1 << i) for i in range(m)], dtype=np.uint64).reshape(m, 4)

    def domain(self, num_elements, shift=None):
        d = _log2(num_elements)
        return Domain(self, ADDITIVE, basis=self.standard_basis(d), shift=np.zeros(4, dtype=np.uint64) if shift is None else shift)

    @staticmethod
    def _int(a):
        w = np.asarray(a, dtype=np.uint64).reshape(-1)
        return sum(int(w[k]) << (64 * k) for k in range(4))

    @staticmethod
    def _elem(v):
        return np.array([(v >> (64 * k)) & GF128._MASK for k in range(4)], dtype=np.uint64)

    @staticmethod
    def _mul(a, b):
        r = 0
        while b:
            if b & 1:
                r ^= a
            b >>= 1
            a <<= 1
            if a >> 256:
                a ^= (1 << 256) | 0x425
        return r

    def zero(self):
        return np.zeros(4, dtype=np.uint64)

    def inv(self, a, lib):
        return lib.gf256_inverse_host(a)

    def squeeze(self, hashchain, n):
        """blake2b_FieldT_randomness_extractor for a binary field of 32 bytes (blake2b.tcc:162-185, 231-257): element i = keyed
        BLAKE2b(state || index, key = i, 32 bytes), the four raw words."""
        hashchain.squeeze_index += 1
        msg = hashchain.state + hashchain.squeeze_index.to_bytes(8, "little")
        out = np.zeros((n, 4), dtype=np.uint64)
        for i in range(n):
            out[i] = np.frombuffer(hashlib.blake2b(msg, digest_size=32, key=i.to_bytes(8, "little")).digest(), dtype="<u8")
        return out

    def fri_domains(self, domain, localization, lib):
        """FRI_protocol::compute_domains, additive branch (fri_ldt.tcc:310-338), by the library's host-side helper."""
        chain = lib.fri_additive_domains_gf256(domain.basis, domain.shift, localization)
        return [domain] + [Domain(self, ADDITIVE, basis=b, shift=s) for b, s in chain[1:]]


class EdwardsFr:
    """libff::edwards_Fr (181 bits, 3 Montgomery limbs), multiplicative arm."""
    name, additive, elem_bytes, words, soundness_bits = "edwards_Fr", False, 24, 3, 180
    P, GENERATOR = la.EDWARDS_FR_MODULUS, la.EDWARDS_FR_GENERATOR
    # the transforms and the fold call the C entry itself (iopx_*): DeviceOps passes the words as pointers
    entries = {
        "FFT": ("iopx_mul_fft_fp3_dev", {}),
        "IFFT": ("iopx_mul_ifft_fp3_dev", {}),
        "IFFT_of_known_degree": ("iopx_mul_ifft_known_degree_fp3_dev", {}),
        "fold": ("iopx_fri_fold_mul_fp3_dev", {}),
        "ldt_combine": ("ldt_combine_multiplicative_dev", {}),
        "rowcheck": ("rowcheck_multiplicative_dev", {}),
        "fz": ("fz_multiplicative_dev", {}),
        "sumcheck_g": ("sumcheck_g_multiplicative_dev", {}),
        "lincheck": ("lincheck_dev", {"prime_field": True}),
        "lincomb": ("lincomb_dev", {"prime_field": True}),
        "lincomb_affine": ("lincomb_affine_dev", {"prime_field": True}),
        "sub": ("fp3_sub_dev", {}),
        "mul": ("fp3_mul_dev", {}),
        "inv": ("field_inv_dev", {"prime_field": True}),
        "pow_table": ("fp3_pow_table_dev", {}),
        "spmv": ("spmv_dev", {"prime_field": True}),
        "div": ("field_div_dev", {"prime_field": True}),
        "domain_offsets": ("domain_offsets_multiplicative_dev", {}),
        "vanishing_evals": ("vanishing_evals_multiplicative_dev", {}),
        "rational_combine": ("rational_combine_dev", {"prime_field": True}),
        "rational_sumcheck_constraint": ("rational_sumcheck_constraint_multiplicative_dev", {}),
        "poly_div_vanishing": ("poly_div_vanishing_multiplicative_dev", {}),
    }

    def domain(self, num_elements, shift=None):
        return Domain(self, MULTIPLICATIVE, shift=1 if shift is None else shift, log_n=_log2(num_elements))

    def to_int(self, words):
        v = int(words[0]) | (int(words[1]) << 64) | (int(words[2]) << 128)
        return v * pow(1 << 192, -1, self.P) % self.P

    def from_int(self, v):
        return la.edwards_to_montgomery([int(v) % self.P])[0]

    def subgroup_generator(self, log_order):
        """multiplicative_generator^((p - 1) / 2^log_order) (subgroup.tcc:55-59)"""
        return la.edwards_subgroup_generator(log_order)

    def zero(self):
        return np.zeros(3, dtype=np.uint64)

    def mul(self, a, b):
        return self.from_int(self.to_int(a) * self.to_int(b))

    def add(self, a, b):
        return self.from_int(self.to_int(a) + self.to_int(b))

    def sub(self, a, b):
        return self.from_int(self.to_int(a) - self.to_int(b))

    def neg(self, a):
        return self.from_int(-self.to_int(a))

    def one(self):
        return self.from_int(1)

    def inv(self, a, lib=None):
        return self.from_int(pow(self.to_int(a), -1, self.P))

    def vanishing_eval(self, domain, x, lib=None):
        """Z_S(x) = x^|S| - shift^|S| (vanishing_polynomial.tcc:14-25)."""
        return self.from_int(pow(self.to_int(x), domain.size, self.P) - pow(domain.shift_int, domain.size, self.P))

    def vanishing_derivative(self, domain, x, lib=None):
        """|S| x^(|S| - 1) (vanishing_polynomial.tcc:57-62)."""
        return self.from_int(domain.size * pow(self.to_int(x), domain.size - 1, self.P))

    def element_in_domain(self, domain, x):
        return pow(self.to_int(x) * pow(domain.shift_int, -1, self.P) % self.P, domain.size, self.P) == 1

    def squeeze(self, hashchain, n):
        """blake2b_FieldT_randomness_extractor for Fp (blake2b.tcc:187-257): keyed BLAKE2b straight into mont_repr, bits above
        the modulus MSB cleared, retry with key += num_elements until below p."""
        hashchain.squeeze_index += 1
        msg = hashchain.state + hashchain.squeeze_index.to_bytes(8, "little")
        out = np.zeros((n, 3), dtype=np.uint64)
        mask = (1 << self.P.bit_length()) - 1
        for i in range(n):
            key = i
            while True:
                raw = int.from_bytes(hashlib.blake2b(msg, digest_size=24, key=key.to_bytes(8, "little")).digest(), "little") & mask
                key += n
                if raw < self.P:
                    break
            out[i] = [(raw >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(3)]
        return out

    def fri_domains(self, domain, localization, lib=None):
        """fri_ldt.tcc:292-308: size >>= eta, shift <- shift^(2^eta)."""
        out, sh, logn = [domain], domain.shift_int, domain.dim
        for eta in localization:
            sh, logn = pow(sh, 1 << eta, self.P), logn - eta
            out.append(Domain(self, MULTIPLICATIVE, shift=sh, log_n=logn))
        return out


def _ldt_combine_bn128(lib, d_oracles, degrees, random_coefficients, log_n, gen, shift, d_out):
    """Library.ldt_combine_bn128_dev takes the generator last, unlike ldt_combine_multiplicative_dev: the one entry whose order is adapted."""
    lib.ldt_combine_bn128_dev(d_oracles, degrees, random_coefficients, log_n, shift, d_out, gen=gen)


class AltBn128Fr(EdwardsFr):
    """libff::alt_bn128_Fr (254 bits, 4 Montgomery limbs, x * 2^256 mod r), multiplicative arm: the device operators of the
    protocol layer.  No prover runs over it yet: challenge sampling (the hashchain extractor into this field) is not here."""
    name, additive, elem_bytes, soundness_bits, words = "alt_bn128_Fr", False, 32, 253, 4
    P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    GENERATOR, TWO_ADICITY = 5, 28
    # the transforms and the fold call the C entry itself, as over edwards_Fr
    entries = {
        "FFT": ("iopx_mul_fft_bn128_dev", {}),
        "IFFT": ("iopx_mul_ifft_bn128_dev", {}),
        "IFFT_of_known_degree": ("iopx_mul_ifft_known_degree_bn128_dev", {}),
        "fold": ("iopx_fri_fold_mul_bn128_dev", {}),
        "ldt_combine": (_ldt_combine_bn128, {}),
        "rowcheck": ("bn128_rowcheck_dev", {}),
        "fz": ("bn128_fz_dev", {}),
        "sumcheck_g": ("bn128_sumcheck_g_dev", {}),
        "lincheck": ("bn128_lincheck_dev", {}),
        "lincomb": ("bn128_lincomb_dev", {}),
        "lincomb_affine": ("bn128_lincomb_affine_dev", {}),
        "sub": ("bn128_sub_dev", {}),
        "mul": ("bn128_mul_dev", {}),
        "inv": ("bn128_inv_dev", {}),
        "pow_table": ("bn128_pow_table_dev", {}),
        "spmv": ("bn128_spmv_dev", {}),
        "div": ("bn128_div_dev", {}),
        "domain_offsets": ("bn128_domain_offsets_dev", {}),
        "vanishing_evals": ("bn128_vanishing_evals_dev", {}),
        "rational_combine": ("bn128_rational_combine_dev", {}),
        "rational_sumcheck_constraint": ("bn128_rational_sumcheck_constraint_dev", {}),
        "poly_div_vanishing": ("bn128_poly_div_vanishing_dev", {}),
    }

    def to_int(self, words):
        v = sum(int(w) << (64 * k) for k, w in enumerate(np.asarray(words, dtype=np.uint64).reshape(4)))
        return v * pow(1 << 256, -1, self.P) % self.P

    def from_int(self, v):
        m = int(v) % self.P * (1 << 256) % self.P
        return np.array([(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)

    def zero(self):
        return np.zeros(4, dtype=np.uint64)

    def subgroup_generator(self, log_order):
        """multiplicative_generator^((r - 1) / 2^log_order) (subgroup.tcc:55-59)"""
        if log_order > self.TWO_ADICITY:
            raise ValueError("log_order %d exceeds the 2-adicity of alt_bn128 Fr" % log_order)
        return self.from_int(pow(self.GENERATOR, (self.P - 1) >> log_order, self.P))

    def squeeze(self, hashchain, n):
        raise NotImplementedError("challenge sampling into alt_bn128 Fr belongs to the prover over this field")


class MerkleTree:
    """A BCS Merkle tree resident on the device: (2L - 1, 32) uint8 nodes in heap order (merkle_tree.tcc:92-229)."""

    def __init__(self, lib, nodes, num_leaves):
        self.lib, self.nodes, self.num_leaves = lib, nodes, num_leaves

    def root(self):
        """merkle_tree::get_root, read on the library's stream."""
        return self.lib.read_digest(self.nodes.data_ptr())

    def membership_proof(self, leaf_positions):
        """merkle_tree::get_set_membership_proof (merkle_tree.tcc:242-336): the auxiliary hashes as a (count, 32) uint8 array."""
        return self.lib.get_set_membership_proof_dev(self.nodes.data_ptr(), self.num_leaves, leaf_positions)


class DeviceOps:
    """The device operators of the path: one body each, for every field.  What differs between the fields is data: `field.words` and
    `field.elem_bytes` size the vectors, `field.entries` names the entry of each operator, and a Domain hands over its own arguments
    (`Domain.args`, `Domain.sub_args`).  Vectors are (count, field.words) int64 torch tensors on the device the library is bound to; every
    call enqueues on the library's stream and returns without synchronising."""

    def __new__(cls, lib, torch, device, field, *args, **kwargs):
        # alt_bn128 Fr, GF(2^64), GF(2^128) and GF(2^256) have a class of their own (below); GF(2^192) and edwards_Fr run this class as it is.  Four words
        # are alt_bn128 Fr or GF(2^256): field.additive tells them apart.  Only DeviceOps itself is redirected: a subclass (the sharded operators of
        # libiop_amd/dist.py) is built as asked, and __init__ refuses the field there
        if cls is DeviceOps and field.words == 4 and not field.additive:
            cls = AltBn128DeviceOps
        if cls is DeviceOps and field.words == 4 and field.additive:
            cls = GF256DeviceOps
        if cls is DeviceOps and field.words == 1:
            cls = GF64DeviceOps
        if cls is DeviceOps and field.words == 2:
            cls = GF128DeviceOps
        return object.__new__(cls)

    def __init__(self, lib, torch, device, field):
        self.lib, self.torch, self.device, self.field = lib, torch, device, field
        if field.words == 4 and field.additive and not isinstance(self, GF256DeviceOps):
            raise NotImplementedError("%s: no operators over a four-word binary field (gf256 runs on one GPU, through DeviceOps)" % type(self).__name__)
        if field.words == 4 and not field.additive and not isinstance(self, AltBn128DeviceOps):
            raise NotImplementedError("%s: no operators over a four-word field (alt_bn128 Fr runs on one GPU, through DeviceOps)" % type(self).__name__)
        if field.words == 1 and not isinstance(self, GF64DeviceOps):
            raise NotImplementedError("%s: no operators over a one-word field (gf64 runs on one GPU, through DeviceOps)" % type(self).__name__)
        if field.words == 2 and not isinstance(self, GF128DeviceOps):
            raise NotImplementedError("%s: no operators over a two-word field (gf128 runs on one GPU, through DeviceOps)" % type(self).__name__)
        # The provers interleave torch ops (copies, index assignments, torch.cat, buffers recycled by the caching allocator) with
        # library kernels WITHOUT host synchronisation: that is only ordered when both enqueue on the same stream.  Refuse the
        # unshared configuration instead of racing (libiop_amd/dist.py's collectives have their own host-synchronised fallback).
        dev = torch.device(device) if not isinstance(device, torch.device) else device
        if dev.type == "cuda" and not lib.shares_stream_with(torch, dev):
            raise RuntimeError("DeviceOps: the library must enqueue on torch's current stream — call "
                               "lib.set_stream(torch.cuda.current_stream().cuda_stream) before constructing the operators")

    def _call(self, op, *args, **kwargs):
        """The field's entry for `op` on `args`: a Library method by name, a C entry by name (iopx_*) or, for the one method whose argument
        order differs from its twins', the function that adapts it.  A name the field's table lacks raises: nothing falls through to another
        field's entry (libiop_amd/cpp/field_ops.hpp does the same)."""
        if op not in self.field.entries:
            raise NotImplementedError("%s: DeviceOps.%s has no entry over this field" % (self.field.name, op))
        target, fixed = self.field.entries[op]
        if callable(target):
            target(self.lib, *args, **fixed, **kwargs)
        elif target.startswith("iopx_"):                                 # the C entry itself: integers and addresses as they are, words as pointers
            self.lib._check(getattr(self.lib.c, target)(*[a if isinstance(a, int) else _p(a) for a in args]))
        else:
            getattr(self.lib, target)(*args, **fixed, **kwargs)

    # ---- layout: one GPU holds every vector whole (libiop_amd/dist.py overrides these for contiguous-coset sharding) ----
    def local_size(self, domain):
        return domain.size

    def mark_codeword_domain(self, domain):
        return domain

    def mark_fri_domains(self, domains, localization):
        return domains

    def query_responses(self, d_oracles, domain, positions):
        """values[p][k] = oracle_k[positions[p]] (bcs_prover.tcc:187-197) as a (positions, oracles, field.words) uint64 array."""
        return self.lib.query_responses_dev([t.data_ptr() for t in d_oracles], self.field.elem_bytes, domain.size, positions)

    def empty(self, n):
        return self.torch.empty((max(int(n), 1), self.field.words), dtype=self.torch.int64, device=self.device)[: int(n)]

    def upload(self, host_words):
        a = np.ascontiguousarray(host_words, dtype=np.uint64).reshape(-1, self.field.words)
        t = self.empty(a.shape[0])
        if a.shape[0]:
            self.lib.h2d(t.data_ptr(), a)
        return t

    def upload_raw(self, arr, dtype):
        a = np.ascontiguousarray(arr)
        t = self.torch.empty((max(a.size, 1),), dtype=dtype, device=self.device)
        if a.size:
            self.lib.h2d(t.data_ptr(), a)
        return t

    def download(self, t, count=None):
        n = t.shape[0] if count is None else count
        out = np.empty((n, self.field.words), dtype=np.uint64)
        if n:
            self.lib.d2h(out, t.data_ptr())
        return out

    # ---- transforms ----
    def FFT(self, d_coeffs, n_coeffs, domain):
        """FFT_over_field_subset (fft.tcc:407-419)."""
        out = self.empty(domain.size)
        self._call("FFT", d_coeffs.data_ptr(), int(n_coeffs), *domain.args(), out.data_ptr())
        return out

    def FFT_batch(self, d_coeffs_list, n_coeffs, domain):
        """Several polynomials with the same coefficient count onto one domain: one batched extension where the field has it."""
        if "LDE_batch" in self.field.entries and len(d_coeffs_list) > 1:
            outs = [self.empty(domain.size) for _ in d_coeffs_list]
            d = max(int(n_coeffs) - 1, 0).bit_length()
            self._call("LDE_batch", [t.data_ptr() for t in d_coeffs_list], int(n_coeffs), *domain.args(), 0, 1 << (domain.dim - d),
                       [o.data_ptr() for o in outs])
            return outs
        return [self.FFT(t, n_coeffs, domain) for t in d_coeffs_list]

    def IFFT(self, d_evals, domain):
        """IFFT_over_field_subset (fft.tcc:421-433)."""
        out = self.empty(domain.size)
        self._call("IFFT", d_evals.data_ptr(), *domain.args(), out.data_ptr())
        return out

    def IFFT_batch(self, d_evals_list, domain):
        if "IFFT_batch" in self.field.entries and len(d_evals_list) > 1:
            packed = self.empty(domain.size * len(d_evals_list))
            for k, t in enumerate(d_evals_list):
                packed[k * domain.size:(k + 1) * domain.size].copy_(t)
            return self.IFFT_batch_packed(packed, len(d_evals_list), domain)
        return [self.IFFT(t, domain) for t in d_evals_list]

    def IFFT_batch_packed(self, packed, batch, domain):
        """`batch` vectors stored back to back in one tensor: one batched inverse transform (phase-1 passes shared) where the field has it."""
        n = domain.size
        if "IFFT_batch" in self.field.entries and batch > 1:
            out = self.empty(n * batch)
            self._call("IFFT_batch", packed.data_ptr(), batch, *domain.args(), out.data_ptr())
            return [out[k * n:(k + 1) * n] for k in range(batch)]
        return [self.IFFT(packed[k * n:(k + 1) * n], domain) for k in range(batch)]

    def reextend_packed(self, packed, batch, eval_domain, codeword_domain):
        """FFT_over_field_subset(IFFT_over_field_subset(v, eval_domain), codeword_domain) for `batch` vectors stored back to back.
        With a fused entry, and the evaluation domain spanned by the first basis vectors of the codeword domain, the coefficient form is
        skipped (iopx_add_reextend_gf192_batch_dev).  With a coset-range extension alone, the inverse transforms are followed by one
        extension per vector onto this process's cosets.  Otherwise the two transforms run one after the other."""
        n, d = eval_domain.size, eval_domain.dim
        if "reextend_batch" in self.field.entries and np.array_equal(eval_domain.basis, codeword_domain.basis[:d]):
            lo, cnt = self._coset_range(codeword_domain, d)
            outs = [self.empty(cnt << d) for _ in range(batch)]
            self._call("reextend_batch", packed.data_ptr(), batch, codeword_domain.basis, d, eval_domain.shift, codeword_domain.shift, lo, cnt,
                       [o.data_ptr() for o in outs])
            return outs
        if "LDE" in self.field.entries:
            lo, cnt = self._coset_range(codeword_domain, d)
            outs = []
            for coeffs in self.IFFT_batch_packed(packed, batch, eval_domain):
                out = self.empty(cnt << d)
                self._call("LDE", coeffs.data_ptr(), n, *codeword_domain.args(), lo, cnt, out.data_ptr())
                outs.append(out)
            return outs
        return self.FFT_batch(self.IFFT_batch_packed(packed, batch, eval_domain), n, codeword_domain)

    def _coset_range(self, codeword_domain, d):
        """The cosets of span(basis[:d]) this process holds: all of them on one GPU."""
        return 0, 1 << (codeword_domain.dim - d)

    def IFFT_of_known_degree(self, d_evals, degree, domain):
        """IFFT_of_known_degree_over_field_subset (fft.tcc:435-475): 2^ceil(log2 degree) coefficients."""
        k = _log2(degree)
        if domain.additive:
            return self.IFFT(d_evals[: 1 << k], domain.get_subset_of_order(1 << k))
        out = self.empty(1 << k)
        self._call("IFFT_of_known_degree", d_evals.data_ptr(), int(degree), *domain.args(), out.data_ptr())
        return out

    # ---- FRI / Merkle ----
    def fold(self, d_f, domain, coset_size, x_i, next_domain=None):
        """evaluate_next_f_i_over_entire_domain (fri_aux.tcc:5-34)."""
        out = self.empty(domain.size // coset_size)
        self._call("fold", d_f.data_ptr(), *domain.args(), int(coset_size), x_i, out.data_ptr())
        return out

    def solve_pow(self, challenge, pow_bitlen):
        """pow::solve_pow (bcs/pow.tcc:67-103): the first passing candidate in the reference's order."""
        return self.lib.solve_pow(challenge, pow_bitlen)

    def merkle_tree(self, d_oracles, domain, coset_size):
        """construct_with_leaves_serialized_by_cosets + compute_inner_nodes over device-resident oracles."""
        leaves = domain.size // coset_size
        nodes = self.torch.empty((2 * leaves - 1, 32), dtype=self.torch.uint8, device=self.device)
        self.lib.merkle_tree_dev([t.data_ptr() for t in d_oracles], self.field.elem_bytes, domain.size, coset_size, nodes.data_ptr(),
                                 domain_type=domain.domain_type)
        return MerkleTree(self.lib, nodes, leaves)

    # ---- virtual oracles ----
    def rowcheck(self, d_az, d_bz, d_cz, codeword_domain, constraint_domain):
        out = self.empty(codeword_domain.size)
        self._call("rowcheck", d_az.data_ptr(), d_bz.data_ptr(), d_cz.data_ptr(), *codeword_domain.args(), constraint_domain.dim,
                   constraint_domain.shift, out.data_ptr())
        return out

    def fz(self, d_fw, d_f1v, codeword_domain, input_domain):
        out = self.empty(codeword_domain.size)
        self._call("fz", d_fw.data_ptr(), d_f1v.data_ptr(), *codeword_domain.args(), *input_domain.sub_args(), out.data_ptr())
        return out

    def sumcheck_g(self, d_f, d_h, codeword_domain, summation_domain, claimed_sum):
        out = self.empty(codeword_domain.size)
        self._call("sumcheck_g", d_f.data_ptr(), d_h.data_ptr(), *codeword_domain.args(), *summation_domain.sub_args(), claimed_sum, out.data_ptr())
        return out

    def lincheck(self, d_fz, d_mz, r_mz, d_p1, d_p2, n):
        out = self.empty(n)
        self._call("lincheck", d_fz.data_ptr(), [t.data_ptr() for t in d_mz], r_mz, d_p1.data_ptr(), d_p2.data_ptr(), n, out.data_ptr())
        return out

    def ldt_combine(self, d_oracles, degrees, random_coefficients, domain):
        out = self.empty(domain.size)
        self._call("ldt_combine", [t.data_ptr() for t in d_oracles], degrees, random_coefficients, *domain.args(), out.data_ptr())
        return out

    def lincomb(self, d_oracles, coefficients, n):
        out = self.empty(n)
        self._call("lincomb", [t.data_ptr() for t in d_oracles], coefficients, n, out.data_ptr())
        return out

    # ---- vector-sized steps of the encoded prover ----
    def sub(self, d_a, d_b):
        out = self.empty(d_a.shape[0])
        self._call("sub", d_a.data_ptr(), d_b.data_ptr(), out.data_ptr(), d_a.shape[0])
        return out

    def mul(self, d_a, d_b):
        out = self.empty(d_a.shape[0])
        self._call("mul", d_a.data_ptr(), d_b.data_ptr(), out.data_ptr(), d_a.shape[0])
        return out

    def inv(self, d_a):
        out = self.empty(d_a.shape[0])
        self._call("inv", d_a.data_ptr(), out.data_ptr(), d_a.shape[0])
        return out

    def pow_table(self, count, base, init):
        out = self.empty(count)
        self._call("pow_table", out.data_ptr(), count, base, init)
        return out

    def spmv(self, csr, d_vec, d_out=None, scale=None, accumulate=False):
        out = self.empty(csr.rows) if d_out is None else d_out
        self._call("spmv", csr.d_row_ptr.data_ptr(), csr.d_col.data_ptr(), csr.d_coeff.data_ptr(), csr.rows, d_vec.data_ptr(), out.data_ptr(),
                   scale=scale, accumulate=accumulate)
        return out

    # ---- vector-sized steps of the holographic prover ----
    def div(self, d_num, d_den):
        """d_num / d_den elementwise by batch inversion (d_num None: the inverses)."""
        out = self.empty(d_den.shape[0])
        self._call("div", d_num.data_ptr() if d_num is not None else None, d_den.data_ptr(), out.data_ptr(), d_den.shape[0])
        return out

    def domain_offsets(self, domain, point):
        """point - x over the whole domain."""
        out = self.empty(domain.size)
        self._call("domain_offsets", *domain.args(), point, out.data_ptr())
        return out

    def domain_elements(self, domain):
        """field_subset::all_elements on the device."""
        if domain.additive:
            return self.domain_offsets(domain, self.field.zero())
        return self.pow_table(domain.size, domain.gen, domain.shift)

    def vanishing_evals(self, vanishing_domain, domain, constant):
        """constant - Z_S(x) over the whole domain (S = vanishing_domain)."""
        out = self.empty(domain.size)
        self._call("vanishing_evals", *domain.args(), *vanishing_domain.sub_args(), constant, out.data_ptr())
        return out

    def lagrange_evals(self, x, S, evaldomain):
        """lagrange_polynomial(x, S, normalized = false).evaluations_over_field_subset(evaldomain) (lagrange_polynomial.tcc:66-136):
        (Z_S(x) - Z_S(y)) / (x - y) for y over evaldomain.  The reference patches the position y = x (probability |evaldomain| / |F|
        for a sampled x) with the formal derivative; here that case is refused instead of silently differing."""
        if self.field.element_in_domain(evaldomain, x):
            raise NotImplementedError("the evaluation point lies in the evaluation domain")
        numerator = self.vanishing_evals(S, evaldomain, self.field.vanishing_eval(S, x, self.lib))
        return self.div(numerator, self.domain_offsets(evaldomain, x))

    def lincomb_affine(self, d_oracles, coefficients, constant, n):
        out = self.empty(n)
        self._call("lincomb_affine", [t.data_ptr() for t in d_oracles], coefficients, constant, n, out.data_ptr())
        return out

    def rational_combine(self, d_numerators, d_denominators, coefficients, n):
        """(combined numerator, combined denominator) of sum_i c_i N_i / D_i."""
        N, D = self.empty(n), self.empty(n)
        self._call("rational_combine", [t.data_ptr() for t in d_numerators], [t.data_ptr() for t in d_denominators], coefficients, n,
                   N.data_ptr(), D.data_ptr())
        return N, D

    def rational_sumcheck_constraint(self, d_p, d_N, d_D, codeword_domain, summation_domain, claimed_sum):
        out = self.empty(codeword_domain.size)
        L, K = codeword_domain, summation_domain
        xinv = []
        if L.additive:                                                   # the subspace entry also takes 1 / x over the codeword domain
            if not np.array_equal(K.basis, L.basis[: K.dim]):
                raise ValueError("the summation domain must be spanned by a prefix of the codeword domain's basis")
            xinv = [self.div(None, self.domain_offsets(L, self.field.zero()))]
        self._call("rational_sumcheck_constraint", d_p.data_ptr(), d_N.data_ptr(), d_D.data_ptr(), *[t.data_ptr() for t in xinv], *L.args(), K.dim,
                   K.shift, claimed_sum, out.data_ptr())
        return out

    def poly_div_vanishing(self, d_poly, n_coeffs, domain, out=None):
        """polynomial_over_vanishing_polynomial(P, Z_domain).first (written to the head of `out` when given)."""
        out = self.empty(max(n_coeffs - domain.size, 0)) if out is None else out
        if n_coeffs > domain.size:
            self._call("poly_div_vanishing", d_poly.data_ptr(), n_coeffs, *domain.sub_args(), out.data_ptr())
        return out


class AltBn128DeviceOps(DeviceOps):
    """DeviceOps over AltBn128Fr: (count, 4) int64 vectors, the iopx_*_bn128_dev entries of AltBn128Fr.entries.  The field has no batched or
    fused transform, so batches and the re-extension loop over the single-vector ones; a coset range has no alt_bn128 Fr form."""


class GF64DeviceOps(DeviceOps):
    """DeviceOps over GF64: (count, 1) int64 vectors, the iopx_*_gf64 entries of GF64.entries.  It allows what the FRI-only SNARK
    (libiop_amd/fri.py) calls; every other operator of DeviceOps raises NotImplementedError."""


class GF128DeviceOps(DeviceOps):
    """DeviceOps over GF128: (count, 2) int64 vectors, the iopx_*_gf128 entries through GF128.entries.  It allows what the FRI-only SNARK
    (libiop_amd/fri.py) calls; every other operator of DeviceOps raises NotImplementedError."""


class GF256DeviceOps(DeviceOps):
    """DeviceOps over GF256: (count, 4) int64 vectors, the iopx_*_gf256 entries through GF256.entries.  It allows what the FRI-only SNARK
    (libiop_amd/fri.py) calls; every other operator of DeviceOps raises NotImplementedError."""


class GF64AuroraOps(GF64DeviceOps):
    """GF64DeviceOps plus what the Aurora prover (libiop_amd/aurora.py, libiop_amd/bcs.py) calls: the iopx_*_gf64_dev entries of
    libiop_amd/csrc/gfx_ops.h (gf64_ops.hip).  Constructed by name — DeviceOps(...) over GF64 keeps returning GF64DeviceOps.  The operators only Fractal
    calls (div, domain_offsets, domain_elements, vanishing_evals, lagrange_evals, rational_*) keep raising."""


class GF64FractalOps(GF64AuroraOps):
    """GF64AuroraOps plus what the Fractal prover (libiop_amd/fractal.py) calls: the iopx_*_gf64_dev entries of include/libiop_amd_fractal.h.  Constructed
    by name — GF64AuroraOps and DeviceOps(...) over GF64 keep refusing what they refused before."""


class GF128AuroraOps(GF128DeviceOps):
    """GF128DeviceOps plus what the Aurora prover calls: the iopx_*_gf128_dev entries of libiop_amd/csrc/gf128_ops.hip.  Constructed by name —
    DeviceOps(...) over GF128 keeps returning GF128DeviceOps.  The operators only Fractal calls keep raising."""


class GF256AuroraOps(GF256DeviceOps):
    """GF256DeviceOps plus what the Aurora prover calls: the iopx_*_gf256_dev entries of libiop_amd/csrc/gf256_ops.hip.  Constructed by name —
    DeviceOps(...) over GF256 keeps returning GF256DeviceOps.  The operators only Fractal calls keep raising."""


class GF128FractalOps(GF128AuroraOps):
    """GF128AuroraOps plus what the Fractal prover (libiop_amd/fractal.py) calls: the iopx_*_gf128_dev entries of include/libiop_amd_fractal.h.
    Constructed by name — GF128AuroraOps and DeviceOps(...) over GF128 keep refusing what they refused before."""


class GF256FractalOps(GF256AuroraOps):
    """GF256AuroraOps plus what the Fractal prover (libiop_amd/fractal.py) calls: the iopx_*_gf256_dev entries of include/libiop_amd_fractal.h.
    Constructed by name — GF256AuroraOps and DeviceOps(...) over GF256 keep refusing what they refused before."""


_OPERATORS = frozenset(name for name, f in vars(DeviceOps).items() if callable(f) and not name.startswith("__") and name != "_call")
_GF64_FRI = frozenset({"local_size", "mark_codeword_domain", "mark_fri_domains", "query_responses", "empty", "upload", "download", "FFT", "IFFT",
                       "IFFT_of_known_degree", "fold", "solve_pow", "merkle_tree", "ldt_combine"})
_GF64_AURORA = _GF64_FRI | {"upload_raw", "FFT_batch", "IFFT_batch", "IFFT_batch_packed", "reextend_packed", "_coset_range", "rowcheck", "fz",
                            "sumcheck_g", "lincheck", "lincomb", "lincomb_affine", "sub", "mul", "inv", "pow_table", "spmv", "poly_div_vanishing"}


def _allow_only(cls, allowed, why):
    """Every operator of DeviceOps, set on `cls`: the base function where `allowed` names it, otherwise a stub that raises before it looks at
    its arguments, whatever their number.  An operator added to DeviceOps later is refused until a set names it."""
    def refusing(name):
        def op(self, *args, **kwargs):
            raise NotImplementedError(why % name)
        op.__name__ = name
        return op
    if not allowed <= _OPERATORS:
        raise TypeError("not operators of DeviceOps: %s" % sorted(allowed - _OPERATORS))
    for name in _OPERATORS:
        setattr(cls, name, getattr(DeviceOps, name) if name in allowed else refusing(name))


_GF64_WHY = "gf64: DeviceOps.%s has no GF(2^64) entry (the FRI-only SNARK and, through GF64AuroraOps, Aurora are the provers over this field)"
_allow_only(GF64DeviceOps, _GF64_FRI, _GF64_WHY)
_allow_only(GF64AuroraOps, _GF64_AURORA, _GF64_WHY)
_GFX_FRACTAL = _GF64_AURORA | {"div", "domain_offsets", "domain_elements", "vanishing_evals", "lagrange_evals", "rational_combine",
                               "rational_sumcheck_constraint"}
_allow_only(GF64FractalOps, _GFX_FRACTAL, _GF64_WHY)
_allow_only(GF128DeviceOps, _GF64_FRI, "gf128: DeviceOps.%s has no GF(2^128) entry (the FRI-only SNARK is the prover over this field)")
_allow_only(GF256DeviceOps, _GF64_FRI, "gf256: DeviceOps.%s has no GF(2^256) entry (the FRI-only SNARK is the prover over this field)")
_allow_only(GF128AuroraOps, _GF64_AURORA, "gf128: DeviceOps.%s has no GF(2^128) entry (the FRI-only SNARK and, through GF128AuroraOps, Aurora are the provers over this field)")
_allow_only(GF256AuroraOps, _GF64_AURORA, "gf256: DeviceOps.%s has no GF(2^256) entry (the FRI-only SNARK and, through GF256AuroraOps, Aurora are the provers over this field)")
_allow_only(GF128FractalOps, _GFX_FRACTAL, "gf128: DeviceOps.%s has no GF(2^128) entry (the FRI-only SNARK and, through GF128AuroraOps and GF128FractalOps, Aurora and Fractal are the provers over this field)")
_allow_only(GF256FractalOps, _GFX_FRACTAL, "gf256: DeviceOps.%s has no GF(2^256) entry (the FRI-only SNARK and, through GF256AuroraOps and GF256FractalOps, Aurora and Fractal are the provers over this field)")
_allow_only(AltBn128DeviceOps, _OPERATORS - {"_coset_range"}, "DeviceOps.%s: coset ranges belong to the additive re-extension: no alt_bn128 Fr form")


def _p(words):
    return np.ascontiguousarray(words, dtype=np.uint64).ctypes.data_as(la._u64p)
