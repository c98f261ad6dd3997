//go:build mi355x

// The point updates of the SRS ceremony on an MI355X: what package mpcsetup does one ScalarMultiplication after another on
// one core - UpdateMonomialsG1 (A[i] <- rⁱ·A[i], called by Contribute and Seal), the slice cases of UpdateValues (every
// point of a slice by one value) - and the two sums that SameRatioMany pairs (linearCombinationsG1/G2), as three entries:
//
//	gmsm_update_monomials      out[i] = rⁱ·A[i]; the powers are made on the device
//	gmsm_batch_scale           out[i] = s·A[i] (one scalar for all) or sᵢ·A[i]
//	gmsm_linear_combinations   truncated = ∑ rⁱ·A[i], shifted = ∑ rⁱ·A[i+1] over every i that is not the last of its slice
//
// Results are the reference's bit for bit (canonical affine coordinates). Precondition, as for ScalarMultiplication itself:
// the points lie in the r-torsion - Verify subgroup-checks before it forms the linear combinations. Pairings, hashing to G2
// and the proof of knowledge stay with the package.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_mpcsetup_abi.py checks tags, package, symbols and arities.
package mpcsetup

/*
#cgo CFLAGS: -I${SRCDIR}/../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"unsafe"

	curve "github.com/consensys/gnark-crypto/ecc/bls12-381"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
)

// group ids of include/gmsm.h for this curve
const (
	gmsmG1 = C.int(C.GMSM_BLS12_381_G1)
	gmsmG2 = C.int(C.GMSM_BLS12_381_G2)
)

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

func updateMonomials(group C.int, points unsafe.Pointer, n int, r *fr.Element) error {
	if rc := C.gmsm_update_monomials(group, (*C.uint64_t)(points), nil, C.size_t(n), (*C.uint64_t)(unsafe.Pointer(r)), nil, (*C.uint64_t)(points), nil); rc != 0 {
		return gmsmErr()
	}
	return nil
}

func scale(group C.int, points unsafe.Pointer, n int, s *fr.Element) error {
	if rc := C.gmsm_batch_scale(group, (*C.uint64_t)(points), nil, C.size_t(n), (*C.uint64_t)(unsafe.Pointer(s)), nil, 1, nil, (*C.uint64_t)(points), nil); rc != 0 {
		return gmsmErr()
	}
	return nil
}

func linearCombinations(group C.int, points unsafe.Pointer, n int, r *fr.Element, ends []int, truncated, shifted unsafe.Pointer) error {
	cends := make([]C.size_t, len(ends)+1)
	for i := range ends {
		cends[i] = C.size_t(ends[i])
	}
	if rc := C.gmsm_linear_combinations(group, (*C.uint64_t)(points), nil, C.size_t(n), &cends[0], C.size_t(len(ends)), (*C.uint64_t)(unsafe.Pointer(r)), nil, (*C.uint64_t)(truncated), (*C.uint64_t)(shifted)); rc != 0 {
		return gmsmErr()
	}
	return nil
}

// UpdateMonomialsG1Device is UpdateMonomialsG1(A, r) on the device, in place. len(A) < 2 is an error (the reference panics).
func UpdateMonomialsG1Device(A []curve.G1Affine, r *fr.Element) error {
	if len(A) < 2 {
		return errors.New("mpcsetup: UpdateMonomialsG1 needs at least 2 points")
	}
	return updateMonomials(gmsmG1, unsafe.Pointer(&A[0]), len(A), r)
}

// UpdateMonomialsG2Device is A[i] <- rⁱ·A[i] over G2 points, in place.
func UpdateMonomialsG2Device(A []curve.G2Affine, r *fr.Element) error {
	if len(A) < 2 {
		return errors.New("mpcsetup: UpdateMonomialsG2 needs at least 2 points")
	}
	return updateMonomials(gmsmG2, unsafe.Pointer(&A[0]), len(A), r)
}

// ScaleG1Device is A[i] <- s·A[i], in place: what UpdateValues does to a []G1Affine.
func ScaleG1Device(A []curve.G1Affine, s *fr.Element) error {
	if len(A) == 0 {
		return nil
	}
	return scale(gmsmG1, unsafe.Pointer(&A[0]), len(A), s)
}

// ScaleG2Device is A[i] <- s·A[i], in place: what UpdateValues does to a []G2Affine.
func ScaleG2Device(A []curve.G2Affine, s *fr.Element) error {
	if len(A) == 0 {
		return nil
	}
	return scale(gmsmG2, unsafe.Pointer(&A[0]), len(A), s)
}

// LinearCombinationsG1Device is linearCombinationsG1(A, powers of r, ends); A is not modified.
func LinearCombinationsG1Device(A []curve.G1Affine, r *fr.Element, ends []int) (truncated, shifted curve.G1Affine, err error) {
	if len(A) == 0 {
		return truncated, shifted, errors.New("lengths mismatch")
	}
	var t, s curve.G1Jac
	if err = linearCombinations(gmsmG1, unsafe.Pointer(&A[0]), len(A), r, ends, unsafe.Pointer(&t), unsafe.Pointer(&s)); err == nil {
		truncated.FromJacobian(&t)
		shifted.FromJacobian(&s)
	}
	return
}

// LinearCombinationsG2Device is linearCombinationsG2(A, powers of r, ends); A is not modified.
func LinearCombinationsG2Device(A []curve.G2Affine, r *fr.Element, ends []int) (truncated, shifted curve.G2Affine, err error) {
	if len(A) == 0 {
		return truncated, shifted, errors.New("lengths mismatch")
	}
	var t, s curve.G2Jac
	if err = linearCombinations(gmsmG2, unsafe.Pointer(&A[0]), len(A), r, ends, unsafe.Pointer(&t), unsafe.Pointer(&s)); err == nil {
		truncated.FromJacobian(&t)
		shifted.FromJacobian(&s)
	}
	return
}
