//go:build mi355x

// FoldAndCommit and BatchOpen of package fflonk over a resident proving key on an MI355X (fflonk.go:41-141). The reference
// folds every pack on the host, evaluates every polynomial at every z^t on the host and hands shplonk vectors t times
// longer with sets t times larger. Here the packs go to the device as they are:
//
//	gmsm_fflonk_fold_commit   Commit(Fold(pack)) without a folded copy on the host
//	gmsm_fflonk_open_w        given γ: both sets of claimed values, shplonk's w over the folded polynomials - computed as
//	                          ∑ᵢγⁱ Fold(Pⱼ div ∏ₖ(Y-zₖᵗ)), t chains of divisions over the polynomials as given - and W = Commit(w)
//	gmsm_fflonk_open_wprime   given z: W' = Commit(L/(X-z)), the folded polynomials read from the packs in place
//
// The challenges come from shplonk's own deriveChallenge over the extended sets (extendSet of this package), in the order
// shplonk.BatchOpen uses, so proofs are the reference's bit for bit and BatchVerify accepts them unchanged. One departure:
// two equal points in an extended set (zₐᵗ = z_bᵗ, or z = 0 with t > 1) are refused - shplonk's interpolate inverts zero
// there and returns a meaningless proof without an error.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_fflonk_stubs.py checks tags, package, symbols and arities.
package fflonk

/*
#cgo CFLAGS: -I${SRCDIR}/../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"hash"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark-crypto/ecc/bn254/kzg"
	"github.com/consensys/gnark-crypto/ecc/bn254/shplonk"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// flattenPack concatenates the polynomials of a pack; an all-empty pack has no folded polynomial to commit or open.
func flattenPack(p [][]fr.Element, flat []fr.Element, lens []C.size_t) ([]fr.Element, []C.size_t, bool) {
	nonEmpty := false
	for _, q := range p {
		flat = append(flat, q...)
		lens = append(lens, C.size_t(len(q)))
		nonEmpty = nonEmpty || len(q) > 0
	}
	return flat, lens, nonEmpty
}

// FoldAndCommitResident is FoldAndCommit(p, pk) over the resident key rk.
func FoldAndCommitResident(p [][]fr.Element, rk *kzg.ResidentProvingKey) (kzg.Digest, error) {
	var res kzg.Digest
	handle, _ := rk.Resident()
	flat, lens, nonEmpty := flattenPack(p, nil, nil)
	if !nonEmpty {
		return res, kzg.ErrInvalidPolynomialSize
	}
	var jac bn254.G1Jac
	if rc := C.gmsm_fflonk_fold_commit(C.uint64_t(handle), (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], C.size_t(len(lens)),
		nil, nil, (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return res, gmsmErr()
	}
	res.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}

// BatchOpenResident is BatchOpen(p, digests, points, hf, pk, dataTranscript...) over the resident key rk.
func BatchOpenResident(p [][][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error) {
	var res OpeningProof
	if len(p) != len(points) {
		return res, ErrNbPolynomialsNbPoints
	}
	if len(p) != len(digests) {
		return res, shplonk.ErrInvalidNumberOfDigests
	}
	if len(p) == 0 {
		return res, kzg.ErrInvalidPolynomialSize
	}
	handle, _ := rk.Resident()

	// the packs, the base points and the layout of the results
	var flat, flatPoints []fr.Element
	var lens []C.size_t
	packSizes := make([]C.size_t, len(p))
	npoints := make([]C.size_t, len(p))
	divisors := make([]int, len(p))
	newPoints := make([][]fr.Element, len(p))
	nbClaimed, sizeW := 0, 0
	var err error
	for i := range p {
		if len(p[i]) == 0 || len(points[i]) == 0 {
			return res, kzg.ErrInvalidPolynomialSize
		}
		var nonEmpty bool
		if flat, lens, nonEmpty = flattenPack(p[i], flat, lens); !nonEmpty {
			return res, kzg.ErrInvalidPolynomialSize
		}
		flatPoints = append(flatPoints, points[i]...)
		packSizes[i] = C.size_t(len(p[i]))
		npoints[i] = C.size_t(len(points[i]))
		divisors[i] = getNextDivisorRMinusOne(len(p[i]))
		if newPoints[i], err = extendSet(points[i], divisors[i]); err != nil {
			return res, err
		}
		nbClaimed += divisors[i] * len(points[i])
		for _, q := range p[i] {
			if sizeW < divisors[i]*len(q) {
				sizeW = divisors[i] * len(q)
			}
		}
	}

	fs := fiatshamir.NewTranscript(hf, "gamma", "z")
	gamma, err := shplonk.DeriveChallenge("gamma", newPoints, digests, fs, dataTranscript...)
	if err != nil {
		return res, err
	}

	claimed := make([]fr.Element, nbClaimed)
	foldedClaimed := make([]fr.Element, nbClaimed)
	w := make([]fr.Element, sizeW)
	var jac bn254.G1Jac
	if rc := C.gmsm_fflonk_open_w(C.uint64_t(handle), (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], &packSizes[0], C.size_t(len(p)),
		(*C.uint64_t)(unsafe.Pointer(&flatPoints[0])), &npoints[0], (*C.uint64_t)(unsafe.Pointer(&gamma)), nil,
		(*C.uint64_t)(unsafe.Pointer(&claimed[0])), (*C.uint64_t)(unsafe.Pointer(&foldedClaimed[0])), (*C.uint64_t)(unsafe.Pointer(&w[0])), nil,
		(*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return res, gmsmErr()
	}
	res.SOpeningProof.W.FromJacobian(&jac)
	res.ClaimedValues = make([][][]fr.Element, len(p))
	res.SOpeningProof.ClaimedValues = make([][]fr.Element, len(p))
	at := 0
	for i := range p {
		m, t := len(points[i]), divisors[i]
		res.ClaimedValues[i] = make([][]fr.Element, t)
		for j := 0; j < t; j++ {
			res.ClaimedValues[i][j] = claimed[at+j*m : at+(j+1)*m : at+(j+1)*m]
		}
		res.SOpeningProof.ClaimedValues[i] = foldedClaimed[at : at+t*m : at+t*m]
		at += t * m
	}

	z, err := shplonk.DeriveChallenge("z", nil, []kzg.Digest{res.SOpeningProof.W}, fs)
	if err != nil {
		return res, err
	}

	if rc := C.gmsm_fflonk_open_wprime(C.uint64_t(handle), (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], &packSizes[0], C.size_t(len(p)),
		(*C.uint64_t)(unsafe.Pointer(&flatPoints[0])), &npoints[0], (*C.uint64_t)(unsafe.Pointer(&foldedClaimed[0])), (*C.uint64_t)(unsafe.Pointer(&gamma)),
		(*C.uint64_t)(unsafe.Pointer(&w[0])), nil, (*C.uint64_t)(unsafe.Pointer(&z)), nil, (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return res, gmsmErr()
	}
	res.SOpeningProof.WPrime.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}
