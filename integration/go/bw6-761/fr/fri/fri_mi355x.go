//go:build mi355x

// The prover of package fr/fri on an MI355X, over MiMC: the layers and one Merkle tree per layer stay in HBM from the first FFT
// to the last path (gmsm_fri_commit, gmsm_fri_fold), every tree is built once instead of twice, and the openings of a round come
// back from one gather launch (gmsm_fri_query). The transcript is the reference's, on the host; proofs are the bytes
// RADIX_2_FRI.New(size, mimc.NewMiMC()) produces, so VerifyProofOfProximity and VerifyOpening accept them unchanged.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_fri_stubs.py checks tags, package, symbols and arities.
package fri

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math/big"
	"math/bits"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr/mimc"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

const gmsmG1 = C.int(C.GMSM_BW6_761_G1)

// ErrDeviceSize is returned for a size below 2: the reference's verifier has no interaction to look at there.
var ErrDeviceSize = errors.New("fri: the size must be at least 2")

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// deviceOracle is the committed polynomial on the device: gmsm_fri_commit over a domain of rho * NextPowerOfTwo(size) points.
type deviceOracle struct {
	domain, handle C.uint64_t
	cardinality    uint64
	nbSteps        int
}

func commitDevice(size uint64, p []fr.Element) (*deviceOracle, error) {
	if size < 2 {
		return nil, ErrDeviceSize
	}
	n := ecc.NextPowerOfTwo(size)
	o := &deviceOracle{cardinality: n * rho, nbSteps: bits.TrailingZeros64(n)}
	if rc := C.gmsm_fft_domain_new(gmsmG1, C.uint64_t(o.cardinality), &o.domain); rc != 0 {
		return nil, gmsmErr()
	}
	q := make([]fr.Element, o.cardinality) // copy(q, p): zero padded, cut at the cardinality
	copy(q, p)
	if rc := C.gmsm_fri_commit(o.domain, (*C.uint64_t)(unsafe.Pointer(&q[0])), nil, C.size_t(len(q)), nil, &o.handle); rc != 0 {
		C.gmsm_fft_domain_release(o.domain)
		return nil, gmsmErr()
	}
	return o, nil
}

func (o *deviceOracle) release() {
	C.gmsm_fri_release(o.handle)
	C.gmsm_fft_domain_release(o.domain)
}

// query returns, per step, the pair of leaves around the position, the sum of the queried leaf and the siblings of its path.
func (o *deviceOracle) query(positions []uint64) (pairs, sums []fr.Element, paths [][]fr.Element, err error) {
	k := len(positions)
	depth := bits.TrailingZeros64(o.cardinality)
	pairs, sums = make([]fr.Element, 2*k), make([]fr.Element, k)
	siblings := make([]fr.Element, k*depth)
	counts := make([]C.uint32_t, k)
	if rc := C.gmsm_fri_query(o.handle, (*C.uint64_t)(unsafe.Pointer(&positions[0])), C.size_t(k), (*C.uint64_t)(unsafe.Pointer(&pairs[0])),
		(*C.uint64_t)(unsafe.Pointer(&sums[0])), (*C.uint64_t)(unsafe.Pointer(&siblings[0])), &counts[0]); rc != 0 {
		return nil, nil, nil, gmsmErr()
	}
	paths = make([][]fr.Element, k)
	for j := range paths {
		paths[j] = siblings[j*depth : j*depth+int(counts[j])]
	}
	return pairs, sums, paths, nil
}

func proofSet(leaf fr.Element, rest []fr.Element) [][]byte {
	res := [][]byte{leaf.Marshal()}
	for i := range rest {
		res = append(res, rest[i].Marshal())
	}
	return res
}

// BuildProofOfProximityDevice is RADIX_2_FRI.New(size, mimc.NewMiMC()).BuildProofOfProximity(p) with the folding, the trees and
// the paths on the device.
func BuildProofOfProximityDevice(size uint64, p []fr.Element) (ProofOfProximity, error) {
	var proof ProofOfProximity
	o, err := commitDevice(size, p)
	if err != nil {
		return proof, err
	}
	defer o.release()
	xis := make([]string, o.nbSteps+1)
	for i := 0; i < o.nbSteps; i++ {
		xis[i] = fmt.Sprintf("x%d", i)
	}
	xis[o.nbSteps] = "s0"
	fs := fiatshamir.NewTranscript(mimc.NewMiMC(), xis...)
	var salt fr.Element
	if err = fs.Bind(xis[0], salt.Marshal()); err != nil {
		return proof, err
	}
	var res Round
	res.Interactions = make([][2]MerkleProof, o.nbSteps)
	roots := make([][]byte, o.nbSteps)
	for i := 0; i < o.nbSteps; i++ {
		var root, xi fr.Element
		if rc := C.gmsm_fri_root(o.handle, C.uint(i), (*C.uint64_t)(unsafe.Pointer(&root))); rc != 0 {
			return proof, gmsmErr()
		}
		roots[i] = root.Marshal()
		if err = fs.Bind(xis[i], roots[i]); err != nil {
			return proof, err
		}
		bxi, err := fs.ComputeChallenge(xis[i])
		if err != nil {
			return proof, err
		}
		xi.SetBytes(bxi)
		// the new layer's root, or the Evaluation after the last fold
		if rc := C.gmsm_fri_fold(o.handle, (*C.uint64_t)(unsafe.Pointer(&xi)), (*C.uint64_t)(unsafe.Pointer(&res.Evaluation))); rc != 0 {
			return proof, gmsmErr()
		}
	}
	if err = fs.Bind(xis[o.nbSteps], res.Evaluation.Marshal()); err != nil {
		return proof, err
	}
	binSeed, err := fs.ComputeChallenge(xis[o.nbSteps])
	if err != nil {
		return proof, err
	}
	var bPos, bCardinality big.Int
	bPos.SetBytes(binSeed)
	bCardinality.SetUint64(o.cardinality)
	bPos.Mod(&bPos, &bCardinality)
	si := radixTwoFri{nbSteps: o.nbSteps}.deriveQueriesPositions(int(bPos.Uint64()), int(o.cardinality))
	positions := make([]uint64, o.nbSteps)
	for i := range positions {
		positions[i] = uint64(si[i])
	}
	pairs, sums, paths, err := o.query(positions)
	if err != nil {
		return proof, err
	}
	for i := 0; i < o.nbSteps; i++ {
		c := si[i] % 2
		numLeaves := o.cardinality >> uint(i)
		res.Interactions[i][c] = MerkleProof{roots[i], proofSet(pairs[2*i+c], paths[i]), numLeaves}
		res.Interactions[i][1-c] = MerkleProof{roots[i], [][]byte{pairs[2*i+1-c].Marshal(), sums[i].Marshal()}, numLeaves}
	}
	proof.Rounds = []Round{res}
	return proof, nil
}

// OpenDevice is RADIX_2_FRI.New(size, mimc.NewMiMC()).Open(p, position) with the transform, the tree and the path on the device.
func OpenDevice(size uint64, p []fr.Element, position uint64) (OpeningProof, error) {
	var res OpeningProof
	o, err := commitDevice(size, p)
	if err != nil {
		return res, err
	}
	defer o.release()
	if position >= o.cardinality {
		return res, ErrRangePosition
	}
	pos := uint64(convertCanonicalSorted(int(position), int(o.cardinality)))
	pairs, _, paths, err := o.query([]uint64{pos})
	if err != nil {
		return res, err
	}
	var root fr.Element
	if rc := C.gmsm_fri_root(o.handle, 0, (*C.uint64_t)(unsafe.Pointer(&root))); rc != 0 {
		return res, gmsmErr()
	}
	res.merkleRoot, res.numLeaves, res.index = root.Marshal(), o.cardinality, pos
	res.ClaimedValue = pairs[pos%2]
	res.ProofSet = proofSet(res.ClaimedValue, paths[0])
	return res, nil
}
