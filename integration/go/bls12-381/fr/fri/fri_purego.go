//go:build !mi355x

// The API of fri_mi355x.go for builds without the tag: the reference's own prover over mimc.NewMiMC() - callers compile either
// way and nothing of the reference changes.
package fri

import (
	"errors"

	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr/mimc"
)

// ErrDeviceSize is returned for a size below 2: the reference's verifier has no interaction to look at there.
var ErrDeviceSize = errors.New("fri: the size must be at least 2")

// BuildProofOfProximityDevice is RADIX_2_FRI.New(size, mimc.NewMiMC()).BuildProofOfProximity(p).
func BuildProofOfProximityDevice(size uint64, p []fr.Element) (ProofOfProximity, error) {
	if size < 2 {
		return ProofOfProximity{}, ErrDeviceSize
	}
	return RADIX_2_FRI.New(size, mimc.NewMiMC()).BuildProofOfProximity(p)
}

// OpenDevice is RADIX_2_FRI.New(size, mimc.NewMiMC()).Open(p, position).
func OpenDevice(size uint64, p []fr.Element, position uint64) (OpeningProof, error) {
	if size < 2 {
		return OpeningProof{}, ErrDeviceSize
	}
	return RADIX_2_FRI.New(size, mimc.NewMiMC()).Open(p, position)
}
