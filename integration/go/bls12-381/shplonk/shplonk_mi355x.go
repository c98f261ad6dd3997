//go:build mi355x

// BatchOpen of package shplonk over a resident proving key on an MI355X (shplonk.go:44-172): polynomial i is opened on its
// own set of points, and what the reference does on the host over full-length vectors - the product by Z_{T\Sᵢ}, the
// division by Z_T, the assembly of L and the division by (X-z) - runs on the device, next to the two commitments:
//
//	gmsm_shplonk_open_w        given γ: the claimed values, w = ∑ᵢγⁱ(fᵢ div Z_{Sᵢ}) (a chain of len(points[i]) divisions by
//	                           (X-s) per polynomial; equal to the reference's w because Z_T = Z_{T\Sᵢ}Z_{Sᵢ}) and W = Commit(w)
//	gmsm_shplonk_open_wprime   given z: W' = Commit(L/(X-z))
//
// The challenges come from the package's own deriveChallenge (shplonk.go:278-308), so proofs are the reference's bit for
// bit and BatchVerify accepts them unchanged. One departure: two equal points inside one points[i] are refused (the
// reference's interpolate inverts zero there and returns a meaningless proof without an error).
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_shplonk_stubs.py checks tags, package, symbols and arities.
package shplonk

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

	"github.com/consensys/gnark-crypto/ecc/bls12-381"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/kzg"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// BatchOpenResident is BatchOpen(polynomials, digests, points, hf, pk, dataTranscript...) over the resident key rk.
func BatchOpenResident(polynomials [][]fr.Element, digests []kzg.Digest, points [][]fr.Element, hf hash.Hash, rk *kzg.ResidentProvingKey, dataTranscript ...[]byte) (OpeningProof, error) {
	var res OpeningProof
	if len(polynomials) != len(points) {
		return res, ErrInvalidNumberOfPoints
	}
	if len(polynomials) != len(digests) {
		return res, ErrInvalidNumberOfDigests
	}
	handle, _ := rk.Resident()

	fs := fiatshamir.NewTranscript(hf, "gamma", "z")
	gamma, err := deriveChallenge("gamma", points, digests, fs, dataTranscript...)
	if err != nil {
		return res, err
	}

	lens := make([]C.size_t, len(polynomials))
	npoints := make([]C.size_t, len(points))
	total, nbPoints, maxLen := 0, 0, 0
	for i := range polynomials {
		if len(polynomials[i]) == 0 || len(points[i]) == 0 {
			return res, kzg.ErrInvalidPolynomialSize
		}
		lens[i] = C.size_t(len(polynomials[i]))
		npoints[i] = C.size_t(len(points[i]))
		total += len(polynomials[i])
		nbPoints += len(points[i])
		if len(polynomials[i]) > maxLen {
			maxLen = len(polynomials[i])
		}
	}
	if len(polynomials) == 0 {
		return res, kzg.ErrInvalidPolynomialSize
	}
	flat := make([]fr.Element, 0, total)
	for _, p := range polynomials {
		flat = append(flat, p...)
	}
	flatPoints := make([]fr.Element, 0, nbPoints)
	for _, s := range points {
		flatPoints = append(flatPoints, s...)
	}
	claimed := make([]fr.Element, nbPoints)
	w := make([]fr.Element, maxLen)

	var jac bls12381.G1Jac
	if rc := C.gmsm_shplonk_open_w(C.uint64_t(handle), (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], C.size_t(len(lens)),
		(*C.uint64_t)(unsafe.Pointer(&flatPoints[0])), &npoints[0], (*C.uint64_t)(unsafe.Pointer(&gamma)), nil,
		(*C.uint64_t)(unsafe.Pointer(&claimed[0])), (*C.uint64_t)(unsafe.Pointer(&w[0])), nil, (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return res, gmsmErr()
	}
	res.W.FromJacobian(&jac)
	res.ClaimedValues = make([][]fr.Element, len(points))
	at := 0
	for i := range points {
		res.ClaimedValues[i] = claimed[at : at+len(points[i]) : at+len(points[i])]
		at += len(points[i])
	}

	z, err := deriveChallenge("z", nil, []kzg.Digest{res.W}, fs)
	if err != nil {
		return res, err
	}

	if rc := C.gmsm_shplonk_open_wprime(C.uint64_t(handle), (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], C.size_t(len(lens)),
		(*C.uint64_t)(unsafe.Pointer(&flatPoints[0])), &npoints[0], (*C.uint64_t)(unsafe.Pointer(&claimed[0])), (*C.uint64_t)(unsafe.Pointer(&gamma)),
		(*C.uint64_t)(unsafe.Pointer(&w[0])), nil, (*C.uint64_t)(unsafe.Pointer(&z)), nil, (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return res, gmsmErr()
	}
	res.WPrime.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}
