//go:build mi355x

// The accumulating-ratio polynomials of package iop, and fr.BatchInvert, on an MI355X: what ratios.go runs as two serial
// prefix products over n elements plus a batch inversion, as three entries:
//
//	gmsm_iop_ratio_copy_constraint   Z of BuildRatioCopyConstraint: factors, prefix products, inversion, expected form
//	gmsm_iop_ratio_shuffled          Z of BuildRatioShuffledVectors
//	gmsm_fr_batch_invert             fr.BatchInvert (0 stays 0)
//
// Results are the reference's bit for bit. The C entries take Lagrange basis only: the checks of the reference (checkSize,
// buildDomain) and its ToLagrange on the inputs run here, through the package's own functions, exactly as in ratios.go. The
// device builds its domain from the cardinality (fr.Generator(n), the default coset shift); a domain made WithShift is
// refused. A permutation value outside [0, len(entries)*n) is an error where the reference panics.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_iop_abi.py checks tags, package, symbols and arities.
package iop

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"sync"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr/fft"
)

// group id of include/gmsm.h for this curve's scalar field
const gmsmG1 = C.int(C.GMSM_BLS12_381_G1)

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// device domains by cardinality, made on first use and kept (the twiddles stay resident like the reference's)
var (
	gmsmDomainsMu sync.Mutex
	gmsmDomains   = map[uint64]C.uint64_t{}
)

func gmsmDomain(domain *fft.Domain) (C.uint64_t, error) {
	shift := fft.GeneratorFullMultiplicativeGroup()
	if !domain.FrMultiplicativeGen.Equal(&shift) {
		return 0, errors.New("gmsm: the device domain uses the default coset shift; this domain was made WithShift")
	}
	gmsmDomainsMu.Lock()
	defer gmsmDomainsMu.Unlock()
	if h, ok := gmsmDomains[domain.Cardinality]; ok {
		return h, nil
	}
	var h C.uint64_t
	if rc := C.gmsm_fft_domain_new(gmsmG1, C.uint64_t(domain.Cardinality), &h); rc != 0 {
		return 0, gmsmErr()
	}
	gmsmDomains[domain.Cardinality] = h
	return h, nil
}

// the polynomials' coefficients, concatenated, and their layouts
func gmsmFlatten(pols []*Polynomial, n int) ([]fr.Element, []C.uint32_t) {
	flat := make([]fr.Element, 0, len(pols)*n)
	layouts := make([]C.uint32_t, len(pols))
	for i, p := range pols {
		flat = append(flat, p.Coefficients()[:n]...)
		layouts[i] = C.uint32_t(p.Layout)
	}
	return flat, layouts
}

func gmsmElems(v []fr.Element) *C.uint64_t { return (*C.uint64_t)(unsafe.Pointer(&v[0])) }

// BuildRatioCopyConstraintDevice is BuildRatioCopyConstraint on the device. Like the reference it leaves the entries in
// Lagrange basis.
func BuildRatioCopyConstraintDevice(entries []*Polynomial, permutation []int64, beta, gamma fr.Element, expectedForm Form, domain *fft.Domain) (*Polynomial, error) {
	if len(entries) == 0 {
		return nil, errors.New("gmsm: no polynomial")
	}
	if err := checkSize(entries); err != nil {
		return nil, err
	}
	n := entries[0].coefficients.Len()
	domain, err := buildDomain(n, domain)
	if err != nil {
		return nil, err
	}
	if len(permutation) < len(entries)*n {
		return nil, errors.New("gmsm: the permutation has fewer than len(entries)*n values")
	}
	for i := range entries {
		entries[i].ToLagrange(domain)
	}
	h, err := gmsmDomain(domain)
	if err != nil {
		return nil, err
	}
	flat, layouts := gmsmFlatten(entries, n)
	coeffs := make([]fr.Element, n)
	if rc := C.gmsm_iop_ratio_copy_constraint(h, gmsmElems(flat), nil, C.size_t(len(entries)), &layouts[0], (*C.int64_t)(unsafe.Pointer(&permutation[0])), nil, (*C.uint64_t)(unsafe.Pointer(&beta)), (*C.uint64_t)(unsafe.Pointer(&gamma)), C.int(expectedForm.Basis), C.int(expectedForm.Layout), nil, gmsmElems(coeffs), nil); rc != 0 {
		return nil, gmsmErr()
	}
	return NewPolynomial(&coeffs, expectedForm), nil
}

// BuildRatioShuffledVectorsDevice is BuildRatioShuffledVectors on the device. Like the reference it leaves the numerators
// and denominators in Lagrange basis.
func BuildRatioShuffledVectorsDevice(numerator, denominator []*Polynomial, beta fr.Element, expectedForm Form, domain *fft.Domain) (*Polynomial, error) {
	if len(numerator) != len(denominator) {
		return nil, ErrNumberPolynomials
	}
	if len(numerator) == 0 {
		return nil, errors.New("gmsm: no polynomial")
	}
	if err := checkSize(numerator, denominator); err != nil {
		return nil, err
	}
	n := numerator[0].coefficients.Len()
	domain, err := buildDomain(n, domain)
	if err != nil {
		return nil, err
	}
	for i := range numerator {
		numerator[i].ToLagrange(domain)
		denominator[i].ToLagrange(domain)
	}
	h, err := gmsmDomain(domain)
	if err != nil {
		return nil, err
	}
	num, numLayouts := gmsmFlatten(numerator, n)
	den, denLayouts := gmsmFlatten(denominator, n)
	coeffs := make([]fr.Element, n)
	if rc := C.gmsm_iop_ratio_shuffled(h, gmsmElems(num), nil, gmsmElems(den), nil, C.size_t(len(numerator)), &numLayouts[0], &denLayouts[0], (*C.uint64_t)(unsafe.Pointer(&beta)), C.int(expectedForm.Basis), C.int(expectedForm.Layout), nil, gmsmElems(coeffs), nil); rc != 0 {
		return nil, gmsmErr()
	}
	return NewPolynomial(&coeffs, expectedForm), nil
}

// BatchInvertDevice is fr.BatchInvert(a) on the device: a new slice, zeros stay zero. It panics where the device fails,
// having no error to return.
func BatchInvertDevice(a []fr.Element) []fr.Element {
	res := make([]fr.Element, len(a))
	if len(a) == 0 {
		return res
	}
	if rc := C.gmsm_fr_batch_invert(gmsmG1, gmsmElems(a), nil, C.size_t(len(a)), nil, gmsmElems(res), nil); rc != 0 {
		panic(gmsmErr())
	}
	return res
}
