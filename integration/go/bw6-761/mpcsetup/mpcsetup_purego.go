//go:build !mi355x

// The same API as mpcsetup_mi355x.go without the device: calls into the package's own functions, so a build without the
// tag behaves exactly like the reference. Two of them need a few lines around the call: the generated UpdateMonomialsG2
// takes []G1Affine, so the G2 update and the one-value slices go through ScalarMultiplication point by point (the loop of
// UpdateValues), and linearCombinationsG1/G2 overwrite both their arguments, so they get copies.
package mpcsetup

import (
	"errors"
	"math/big"

	curve "github.com/consensys/gnark-crypto/ecc/bw6-761"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
)

func powersOf(r *fr.Element, n int) []fr.Element {
	p := make([]fr.Element, n)
	p[0].SetOne()
	for i := 1; i < n; i++ {
		p[i].Mul(&p[i-1], r)
	}
	return p
}

// UpdateMonomialsG1Device is UpdateMonomialsG1(A, r).
func UpdateMonomialsG1Device(A []curve.G1Affine, r *fr.Element) error {
	if len(A) < 2 {
		return errors.New("mpcsetup: UpdateMonomialsG1 needs at least 2 points")
	}
	UpdateMonomialsG1(A, r)
	return nil
}

// UpdateMonomialsG2Device is A[i] <- rⁱ·A[i] over G2 points.
func UpdateMonomialsG2Device(A []curve.G2Affine, r *fr.Element) error {
	if len(A) < 2 {
		return errors.New("mpcsetup: UpdateMonomialsG2 needs at least 2 points")
	}
	var I big.Int
	for i, p := range powersOf(r, len(A)) {
		A[i].ScalarMultiplication(&A[i], p.BigInt(&I))
	}
	return nil
}

// ScaleG1Device is A[i] <- s·A[i].
func ScaleG1Device(A []curve.G1Affine, s *fr.Element) error {
	var I big.Int
	s.BigInt(&I)
	for i := range A {
		A[i].ScalarMultiplication(&A[i], &I)
	}
	return nil
}

// ScaleG2Device is A[i] <- s·A[i].
func ScaleG2Device(A []curve.G2Affine, s *fr.Element) error {
	var I big.Int
	s.BigInt(&I)
	for i := range A {
		A[i].ScalarMultiplication(&A[i], &I)
	}
	return nil
}

// LinearCombinationsG1Device is linearCombinationsG1(A, powers of r, ends) on copies.
func LinearCombinationsG1Device(A []curve.G1Affine, r *fr.Element, ends []int) (truncated, shifted curve.G1Affine, err error) {
	if len(ends) == 0 || ends[len(ends)-1] != len(A) {
		return truncated, shifted, errors.New("lengths mismatch")
	}
	truncated, shifted = linearCombinationsG1(append([]curve.G1Affine(nil), A...), powersOf(r, len(A)), ends)
	return
}

// LinearCombinationsG2Device is linearCombinationsG2(A, powers of r, ends) on copies.
func LinearCombinationsG2Device(A []curve.G2Affine, r *fr.Element, ends []int) (truncated, shifted curve.G2Affine, err error) {
	if len(ends) == 0 || ends[len(ends)-1] != len(A) {
		return truncated, shifted, errors.New("lengths mismatch")
	}
	truncated, shifted = linearCombinationsG2(append([]curve.G2Affine(nil), A...), powersOf(r, len(A)), ends)
	return
}
