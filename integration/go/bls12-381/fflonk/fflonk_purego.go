//go:build !mi355x

// The API of fflonk_mi355x.go for builds without the tag: FoldAndCommit and BatchOpen of the package over the key's host
// copy - callers compile either way and nothing of the reference changes.
package fflonk

import (
	"hash"

	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/kzg"
)

// FoldAndCommitResident is FoldAndCommit(p, pk) (fflonk.go:43-47).
func FoldAndCommitResident(p [][]fr.Element, rk *kzg.ResidentProvingKey) (kzg.Digest, error) {
	_, pk := rk.Resident()
	return FoldAndCommit(p, pk)
}

// BatchOpenResident is BatchOpen(p, digests, points, hf, pk, dataTranscript...) (fflonk.go:77-141).
func BatchOpenResident(p [][][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error) {
	_, pk := rk.Resident()
	return BatchOpen(p, digests, points, hf, pk, dataTranscript...)
}
