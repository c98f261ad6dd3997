//go:build !mi355x

// The same API as ratios_mi355x.go without the device: calls into the package's own functions, so a build without the tag
// behaves exactly like the reference.
package iop

import (
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/fft"
)

// BuildRatioCopyConstraintDevice is BuildRatioCopyConstraint.
func BuildRatioCopyConstraintDevice(entries []*Polynomial, permutation []int64, beta, gamma fr.Element, expectedForm Form, domain *fft.Domain) (*Polynomial, error) {
	return BuildRatioCopyConstraint(entries, permutation, beta, gamma, expectedForm, domain)
}

// BuildRatioShuffledVectorsDevice is BuildRatioShuffledVectors.
func BuildRatioShuffledVectorsDevice(numerator, denominator []*Polynomial, beta fr.Element, expectedForm Form, domain *fft.Domain) (*Polynomial, error) {
	return BuildRatioShuffledVectors(numerator, denominator, beta, expectedForm, domain)
}

// BatchInvertDevice is fr.BatchInvert(a).
func BatchInvertDevice(a []fr.Element) []fr.Element {
	return fr.BatchInvert(a)
}
