//go:build mi355x

// The rest of package iop on an MI355X: the basis changes of Polynomial, its Evaluate, and DivideByXMinusOne, as three entries:
//
//	gmsm_iop_to_basis                ToLagrange / ToCanonical / ToLagrangeCoset, in place, grow included
//	gmsm_iop_evaluate                Evaluate: Horner in Canonical basis, barycentric in the Lagrange bases
//	gmsm_iop_divide_by_x_minus_one   DivideByXMinusOne: the gather, 1/(X^n - 1) on the big coset, FFTInverse(DIT, OnCoset)
//
// Results are the reference's bit for bit, with what polynomial.go does around the transforms kept here: grow, the coset that
// ToLagrangeCoset records, the basis check of DivideByXMinusOne. Domain handles come from gmsmDomain (ratios_mi355x.go): the
// device builds its domain from the cardinality, a domain made WithShift is refused. Three things to know, stated in gmsm.h:
// Evaluate of a Lagrange-basis polynomial at a point of its domain is 0, as in the reference; a LagrangeCoset polynomial whose
// coset was never set is evaluated at 0, as in the reference; a shift outside 0..5, where the reference multiplies x by an
// element it never initialised, is refused (EvaluateDevice panics with the entry's text). The methods panic where the device
// fails, having no error to return.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_iop_poly_abi.py checks tags, package, symbols and arities.
package iop

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/fft"
)

// the switch of ToLagrange / ToCanonical / ToLagrangeCoset on the device: the entry zeroes what grow appended, runs the
// reference's transforms for (p.Form, basis) and reports the layout they leave
func (p *Polynomial) gmsmToBasis(d *fft.Domain, basis Basis) *Polynomial {
	h, err := gmsmDomain(d)
	if err != nil {
		panic(err)
	}
	n := p.coefficients.Len()
	if n > int(d.Cardinality) {
		panic(errors.New("gmsm: the polynomial is longer than the domain"))
	}
	p.grow(int(d.Cardinality))
	var layout C.int
	if rc := C.gmsm_iop_to_basis(h, gmsmElems(*p.coefficients), nil, C.size_t(n), C.int(p.Basis), C.int(p.Layout), C.int(basis), nil, &layout); rc != 0 {
		panic(gmsmErr())
	}
	p.Basis = basis
	p.Layout = Layout(layout)
	return p
}

// ToLagrangeDevice is ToLagrange on the device.
func (p *Polynomial) ToLagrangeDevice(d *fft.Domain) *Polynomial {
	return p.gmsmToBasis(d, Lagrange)
}

// ToCanonicalDevice is ToCanonical on the device.
func (p *Polynomial) ToCanonicalDevice(d *fft.Domain) *Polynomial {
	return p.gmsmToBasis(d, Canonical)
}

// ToLagrangeCosetDevice is ToLagrangeCoset on the device. Like the reference it records the coset (cosetTable[1], the
// domain's FrMultiplicativeGen) whatever the basis p is in.
func (p *Polynomial) ToLagrangeCosetDevice(d *fft.Domain) *Polynomial {
	p.coset.Set(&d.FrMultiplicativeGen)
	return p.gmsmToBasis(d, LagrangeCoset)
}

// EvaluateDevice is Evaluate on the device.
func (p *Polynomial) EvaluateDevice(x fr.Element) fr.Element {
	var res fr.Element
	layout := C.uint32_t(p.Layout)
	if rc := C.gmsm_iop_evaluate(gmsmG1, gmsmElems(*p.coefficients), nil, 1, C.size_t(p.coefficients.Len()), C.size_t(p.size), C.int(p.Basis), &layout, C.uint(p.shift), (*C.uint64_t)(unsafe.Pointer(&p.coset)), (*C.uint64_t)(unsafe.Pointer(&x)), nil, (*C.uint64_t)(unsafe.Pointer(&res))); rc != 0 {
		panic(gmsmErr())
	}
	return res
}

// DivideByXMinusOneDevice is DivideByXMinusOne on the device: a is not modified, the result is in Canonical Regular form.
func DivideByXMinusOneDevice(a *Polynomial, domains [2]*fft.Domain) (*Polynomial, error) {
	if a.Basis != LagrangeCoset {
		return nil, ErrMustBeLagrangeCoset
	}
	small, err := gmsmDomain(domains[0])
	if err != nil {
		return nil, err
	}
	big, err := gmsmDomain(domains[1])
	if err != nil {
		return nil, err
	}
	if a.coefficients.Len() != int(domains[1].Cardinality) || a.size != int(domains[0].Cardinality) {
		return nil, errors.New("gmsm: the polynomial's length and size must be the cardinalities of the two domains")
	}
	coeffs := make([]fr.Element, a.coefficients.Len())
	if rc := C.gmsm_iop_divide_by_x_minus_one(small, big, gmsmElems(*a.coefficients), nil, C.int(a.Basis), C.int(a.Layout), C.uint64_t(a.shift), nil, gmsmElems(coeffs), nil); rc != 0 {
		return nil, gmsmErr()
	}
	res := NewPolynomial(&coeffs, Form{Basis: Canonical, Layout: Regular})
	res.size = a.size
	return res, nil
}
