//go:build !mi355x

// The API of kzg_mi355x.go for builds without the tag: a ResidentProvingKey is the plain ProvingKey, every method is the
// package's own function - callers compile either way and nothing of the reference changes.
package kzg

import (
	"hash"
	"io"
	"os"

	"github.com/consensys/gnark-crypto/ecc/bw6-761"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
)

// ResidentProvingKey is the caller's ProvingKey in this build.
type ResidentProvingKey struct{ host ProvingKey }

// NewResidentProvingKey wraps pk (windowTables has no meaning here).
func NewResidentProvingKey(pk ProvingKey, windowTables bool) (*ResidentProvingKey, error) {
	if len(pk.G1) == 0 {
		return nil, ErrMinSRSSize
	}
	return &ResidentProvingKey{host: pk}, nil
}

// ReadDumpResident is (*SRS).ReadDump on the file (kzg/marshal.go:98-113).
func ReadDumpResident(path string, windowTables bool, maxPkPoints ...int) (*ResidentProvingKey, *VerifyingKey, error) {
	f, err := os.Open(path)
	if err != nil {
		return nil, nil, err
	}
	defer f.Close()
	var srs SRS
	if err := srs.ReadDump(f, maxPkPoints...); err != nil {
		return nil, nil, err
	}
	return &ResidentProvingKey{host: srs.Pk}, &srs.Vk, nil
}

// ReadFromResident is (*ProvingKey).ReadFrom, or UnsafeReadFrom without the subgroup checks (kzg/marshal.go:140-158).
func ReadFromResident(r io.Reader, windowTables bool, subgroupCheck bool) (*ResidentProvingKey, int64, error) {
	var pk ProvingKey
	var n int64
	var err error
	if subgroupCheck {
		n, err = pk.ReadFrom(r)
	} else {
		n, err = pk.UnsafeReadFrom(r)
	}
	if err != nil {
		return nil, n, err
	}
	return &ResidentProvingKey{host: pk}, n, nil
}

// Size is the number of points of the key.
func (rk *ResidentProvingKey) Size() int { return len(rk.host.G1) }

// Resident returns 0 (no device handle in this build) and the key itself: what packages built on kzg, such as shplonk,
// need to run the reference's functions over this key.
func (rk *ResidentProvingKey) Resident() (uint64, ProvingKey) { return 0, rk.host }

// Commit is Commit(p, pk) (kzg.go:159-176).
func (rk *ResidentProvingKey) Commit(p []fr.Element, nbTasks ...int) (Digest, error) {
	return Commit(p, rk.host, nbTasks...)
}

// CommitBatch commits one polynomial after the other.
func (rk *ResidentProvingKey) CommitBatch(ps [][]fr.Element) ([]Digest, error) {
	out := make([]Digest, len(ps))
	for i, p := range ps {
		d, err := Commit(p, rk.host)
		if err != nil {
			return nil, err
		}
		out[i] = d
	}
	return out, nil
}

// Open is Open(p, point, pk) (kzg.go:180-205).
func (rk *ResidentProvingKey) Open(p []fr.Element, point fr.Element) (OpeningProof, error) {
	return Open(p, point, rk.host)
}

// BatchOpenSinglePoint is BatchOpenSinglePoint(polynomials, digests, point, hf, pk, dataTranscript...) (kzg.go:246-339).
func (rk *ResidentProvingKey) BatchOpenSinglePoint(polynomials [][]fr.Element, digests []Digest, point fr.Element, hf hash.Hash, dataTranscript ...[]byte) (BatchOpeningProof, error) {
	return BatchOpenSinglePoint(polynomials, digests, point, hf, rk.host, dataTranscript...)
}

// ToLagrangeG1Resident is ToLagrangeG1(coeffs) (utils.go:25-64).
func ToLagrangeG1Resident(coeffs []bw6761.G1Affine) ([]bw6761.G1Affine, error) {
	return ToLagrangeG1(coeffs)
}

// ToLagrange returns ToLagrangeG1(pk.G1[:size]) as a new key.
func (rk *ResidentProvingKey) ToLagrange(size int) (*ResidentProvingKey, error) {
	if size < 0 || size > len(rk.host.G1) {
		return nil, ErrInvalidPolynomialSize
	}
	lag, err := ToLagrangeG1(rk.host.G1[:size])
	if err != nil {
		return nil, err
	}
	return &ResidentProvingKey{host: ProvingKey{G1: lag}}, nil
}

// Release does nothing in this build.
func (rk *ResidentProvingKey) Release() {}
