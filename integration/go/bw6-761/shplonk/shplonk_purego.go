//go:build !mi355x

// The API of shplonk_mi355x.go for builds without the tag: BatchOpen of the package over the key's host copy - callers
// compile either way and nothing of the reference changes.
package shplonk

import (
	"hash"

	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/kzg"
)

// BatchOpenResident is BatchOpen(polynomials, digests, points, hf, pk, dataTranscript...) (shplonk.go:44-172).
func BatchOpenResident(polynomials [][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error) {
	_, pk := rk.Resident()
	return BatchOpen(polynomials, digests, points, hf, pk, dataTranscript...)
}
