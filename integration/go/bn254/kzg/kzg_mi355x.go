//go:build mi355x

// Resident proving key for package kzg on an MI355X: the SRS points live in HBM (gmsm_bases_register / gmsm_bases_register_dump),
// every commitment is one gmsm_multiexp_bases over them - the 64 bytes per point of the proving key cross PCIe once, not once
// per Commit as through the MultiExp drop-in (ecc/bn254/multiexp_mi355x.go), which already serves the package's own
//
//	Commit(p, pk)                       kzg.go:159-176  (res.MultiExp(pk.G1[:len(p)], p, config))
//	Open / BatchOpenSinglePoint         kzg.go:180, :246 (Commit of the quotient)
//
// unchanged; the methods of the same names below do their host arithmetic on the device as well. This file adds a type next to ProvingKey and touches nothing of the reference (kzg_purego.go gives the same API
// over the plain ProvingKey for builds without the tag, so callers compile either way):
//
//	NewResidentProvingKey(pk, tables)   gmsm_bases_register (+ gmsm_bases_precompute: window tables, one bucket set per commitment)
//	ReadDumpResident(path, max...)      SRS.ReadDump's twin (kzg/marshal.go:98-113): Vk through ReadFrom, the []G1Affine memory of
//	                                    the dump streamed from the file into HBM (gmsm_bases_register_dump) - it never exists as
//	                                    host limbs
//	ReadFromResident(r, tables)         (*ProvingKey).ReadFrom's twin (kzg/marshal.go:140-147): the Encoder's default stream - uint32
//	                                    length, then COMPRESSED points - goes to the device as bytes; Y = sqrt(X^3 + b) and the
//	                                    subgroup checks of Decoder.Decode's []G1Affine case (marshal.go of the curve package; bn254's lines 220-277: unsafeComputeY in parallel) run
//	                                    there (gmsm_bases_register_compressed); a raw stream (WriteRawTo) takes
//	                                    gmsm_bases_register_raw. subgroupCheck = false is UnsafeReadFrom (:151-158)
//	(*ResidentProvingKey).Commit        gmsm_multiexp_bases; below MinDevicePoints the package's Commit when the host copy exists
//	(*ResidentProvingKey).CommitBatch   k polynomials of equal length in one call, two MSMs in flight (gmsm_multiexp_bases_batch)
//	(*ResidentProvingKey).Open          kzg.Open: eval + dividePolyByXminusA as a parallel suffix scan on the device, the quotient
//	                                    committed where it is (gmsm_kzg_open)
//	(*ResidentProvingKey).BatchOpenSinglePoint  the claimed values on the device (gmsm_poly_eval), deriveGamma on the host, then
//	                                    the gamma fold, the division and the commitment on the device (gmsm_kzg_open_folded)
//	(*ResidentProvingKey).ToLagrange    ToLagrangeG1(pk.G1[:size]) (utils.go:25-64) on the device, from the resident points to a
//	                                    new resident key (gmsm_bases_to_lagrange); ToLagrangeG1Resident: the same from host points
//	(*ResidentProvingKey).Release       gmsm_bases_release (also the finalizer)
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_stubs.py checks tags, package, symbols and the cited lines. See INTEGRATION.md 2b.
package kzg

/*
#cgo CFLAGS: -I${SRCDIR}/../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../third_party/gmsm/lib
#include <stdlib.h>
#include "gmsm.h"
*/
import "C"

import (
	"encoding/binary"
	"errors"
	"hash"
	"io"
	"math/bits"
	"os"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
)

// compressedFlagMask: every compressed flag value has the top bit of the first byte set and no uncompressed one has
// (marshal.go:26-30: 10 / 11 against 00 / 01 = infinity, which Bytes() writes over a compressed-size buffer - a proving key
// holds no point at infinity; bls12-381/marshal.go:25-35: 100 / 101 / 110 against 000 / 010).
const compressedFlagMask = 0x80

// MinDevicePoints is the shortest polynomial that is committed on the device when a host copy of the key exists
// (same measured crossover as bn254.MinDevicePoints, INTEGRATION.md section 2c).
var MinDevicePoints = 32

// ResidentProvingKey is a ProvingKey whose G1 points are registered with the device.
type ResidentProvingKey struct {
	handle C.uint64_t
	n      int
	host   ProvingKey // the caller's key (shared, not copied); empty after ReadDumpResident
}

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// NewResidentProvingKey copies pk.G1 to the device once. windowTables: also build 2^(c w) P_i for every window next to the
// SRS (gmsm_bases_precompute: 15 copies for BN254 G1 at 2^20; commitments of 2^13..2^21 coefficients then fill one bucket
// set - 2^20: 1.94 -> 1.56 ms - and calls of up to 2^12 need no host-side fold). Call it before the key is shared.
func NewResidentProvingKey(pk ProvingKey, windowTables bool) (*ResidentProvingKey, error) {
	if len(pk.G1) == 0 {
		return nil, ErrMinSRSSize
	}
	rk := &ResidentProvingKey{n: len(pk.G1), host: pk}
	if rc := C.gmsm_bases_register(C.GMSM_BN254_G1, (*C.uint64_t)(unsafe.Pointer(&pk.G1[0])), nil, C.size_t(len(pk.G1)), &rk.handle); rc != 0 {
		return nil, gmsmErr()
	}
	if windowTables {
		if rc := C.gmsm_bases_precompute(rk.handle, 0); rc != 0 {
			C.gmsm_bases_release(rk.handle)
			return nil, gmsmErr()
		}
	}
	runtime.SetFinalizer(rk, func(k *ResidentProvingKey) { k.Release() })
	return rk, nil
}

type countingReader struct {
	r io.Reader
	n int64
}

func (c *countingReader) Read(p []byte) (int, error) {
	k, err := c.r.Read(p)
	c.n += int64(k)
	return k, err
}

// ReadDumpResident reads what (*SRS).WriteDump wrote (kzg/marshal.go:65-95): the VerifyingKey through ReadFrom, as ReadDump
// does, then marker | length | raw []G1Affine memory (utils/unsafe/dump_slice.go:16-32, :80) from the file straight into HBM.
// Like ReadDump it validates nothing. maxPkPoints as in ReadDump.
func ReadDumpResident(path string, windowTables bool, maxPkPoints ...int) (*ResidentProvingKey, *VerifyingKey, error) {
	f, err := os.Open(path)
	if err != nil {
		return nil, nil, err
	}
	defer f.Close()
	var vk VerifyingKey
	cr := &countingReader{r: f}
	if _, err := vk.ReadFrom(cr); err != nil { // ReadFrom reads exactly the key's encoding (an unbuffered decoder)
		return nil, nil, err
	}
	max := 0
	if len(maxPkPoints) > 0 && maxPkPoints[0] > 0 {
		max = maxPkPoints[0]
	}
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	rk := &ResidentProvingKey{}
	var n C.size_t
	var bad C.int64_t
	if rc := C.gmsm_bases_register_dump(C.GMSM_BN254_G1, cpath, C.uint64_t(cr.n), 1, C.size_t(max), 0, &rk.handle, &n, &bad); rc != 0 {
		return nil, nil, gmsmErr()
	}
	rk.n = int(n)
	if windowTables {
		if rc := C.gmsm_bases_precompute(rk.handle, 0); rc != 0 {
			C.gmsm_bases_release(rk.handle)
			return nil, nil, gmsmErr()
		}
	}
	runtime.SetFinalizer(rk, func(k *ResidentProvingKey) { k.Release() })
	return rk, &vk, nil
}

// ReadFromResident reads what (*ProvingKey).WriteTo / WriteRawTo wrote (kzg/marshal.go:16-32): a big-endian uint32 length and
// the points, compressed (the Encoder's default: X and the flag of Y's half, marshal.go:801-823) or raw. The bytes go to the
// device as they are; decompression - the square root per point that Decoder.Decode spreads over the cores (bn254's marshal.go:258-272)
// - and the subgroup checks run there. subgroupCheck = false is (*ProvingKey).UnsafeReadFrom. A stream that mixes both
// encodings (no Encoder writes one) is refused.
func ReadFromResident(r io.Reader, windowTables bool, subgroupCheck bool) (*ResidentProvingKey, int64, error) {
	var hdr [4]byte
	if _, err := io.ReadFull(r, hdr[:]); err != nil {
		return nil, 0, err
	}
	n := int(binary.BigEndian.Uint32(hdr[:]))
	if n == 0 {
		return nil, 4, ErrMinSRSSize
	}
	first := make([]byte, bn254.SizeOfG1AffineCompressed)
	if _, err := io.ReadFull(r, first); err != nil {
		return nil, 4, err
	}
	size := bn254.SizeOfG1AffineCompressed
	compressed := first[0]&compressedFlagMask != 0
	if !compressed {
		size = bn254.SizeOfG1AffineUncompressed
	}
	buf := make([]byte, n*size)
	copy(buf, first)
	if _, err := io.ReadFull(r, buf[len(first):]); err != nil {
		return nil, 4 + int64(len(first)), err
	}
	check := C.int(0)
	if subgroupCheck {
		check = 2
	}
	rk := &ResidentProvingKey{n: n}
	var bad C.int64_t
	var rc C.int
	if compressed {
		rc = C.gmsm_bases_register_compressed(C.GMSM_BN254_G1, (*C.uint8_t)(unsafe.Pointer(&buf[0])), C.size_t(n), check, &rk.handle, &bad)
	} else {
		rc = C.gmsm_bases_register_raw(C.GMSM_BN254_G1, (*C.uint8_t)(unsafe.Pointer(&buf[0])), C.size_t(n), check, &rk.handle, &bad)
	}
	if rc != 0 {
		return nil, 4 + int64(len(buf)), gmsmErr()
	}
	if windowTables {
		if rc := C.gmsm_bases_precompute(rk.handle, 0); rc != 0 {
			C.gmsm_bases_release(rk.handle)
			return nil, 4 + int64(len(buf)), gmsmErr()
		}
	}
	runtime.SetFinalizer(rk, func(k *ResidentProvingKey) { k.Release() })
	return rk, 4 + int64(len(buf)), nil
}

// Size is the number of registered points.
func (rk *ResidentProvingKey) Size() int { return rk.n }

// Resident returns the handle of the registered bases (0 in builds without the mi355x tag) and the host copy of the key
// (empty after ReadDumpResident / ReadFromResident): what packages built on kzg, such as shplonk, need to call the C ABI
// over this key.
func (rk *ResidentProvingKey) Resident() (uint64, ProvingKey) { return uint64(rk.handle), rk.host }

// Commit commits to a polynomial over the resident SRS: Commit(p, pk) of kzg.go:159-176 without the copy of pk.
func (rk *ResidentProvingKey) Commit(p []fr.Element, nbTasks ...int) (Digest, error) {
	if len(p) == 0 || len(p) > rk.n {
		return Digest{}, ErrInvalidPolynomialSize
	}
	if len(p) < MinDevicePoints && len(rk.host.G1) >= len(p) {
		return Commit(p, rk.host, nbTasks...)
	}
	tasks := 0
	if len(nbTasks) > 0 {
		tasks = nbTasks[0]
	}
	var jac bn254.G1Jac
	if rc := C.gmsm_multiexp_bases(rk.handle, (*C.uint64_t)(unsafe.Pointer(&p[0])), C.size_t(len(p)), C.int(tasks),
		(*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		if rc == 2 {
			return Digest{}, errors.New("invalid config: config.NbTasks > 1024")
		}
		return Digest{}, gmsmErr()
	}
	var res bn254.G1Affine
	res.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}

// CommitBatch commits to k polynomials of the same length in one blocking call that keeps two MultiExp in flight (what
// BatchOpenSinglePoint's callers and provers with many wires do one Commit at a time, kzg.go:246): the scalars of polynomial
// i + 1 cross PCIe while polynomial i is being accumulated.
func (rk *ResidentProvingKey) CommitBatch(ps [][]fr.Element) ([]Digest, error) {
	if len(ps) == 0 {
		return nil, nil
	}
	n := len(ps[0])
	if n == 0 || n > rk.n {
		return nil, ErrInvalidPolynomialSize
	}
	flat := make([]fr.Element, 0, n*len(ps))
	for _, p := range ps {
		if len(p) != n {
			return nil, ErrInvalidPolynomialSize
		}
		flat = append(flat, p...)
	}
	jacs := make([]bn254.G1Jac, len(ps))
	if rc := C.gmsm_multiexp_bases_batch(rk.handle, (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, C.size_t(n), C.size_t(len(ps)), nil,
		(*C.uint64_t)(unsafe.Pointer(&jacs[0]))); rc != 0 {
		return nil, gmsmErr()
	}
	runtime.KeepAlive(rk)
	return bn254.BatchJacobianToAffineG1(jacs), nil
}

// Open is Open(p, point, pk) (kzg.go:180-205) over the resident SRS: the claimed value eval(p, point) and the quotient
// dividePolyByXminusA(_p, ClaimedValue, point) are computed on the device and the quotient is committed there
// (gmsm_kzg_open) - it never exists on the host. Below MinDevicePoints the package's Open when the host copy exists.
func (rk *ResidentProvingKey) Open(p []fr.Element, point fr.Element) (OpeningProof, error) {
	if len(p) == 0 || len(p) > rk.n {
		return OpeningProof{}, ErrInvalidPolynomialSize
	}
	if len(p) < MinDevicePoints && len(rk.host.G1) >= len(p) {
		return Open(p, point, rk.host)
	}
	if len(p) == 1 { // Commit of the empty quotient refuses it (kzg.go:197)
		return OpeningProof{}, ErrInvalidPolynomialSize
	}
	var res OpeningProof
	var jac bn254.G1Jac
	if rc := C.gmsm_kzg_open(rk.handle, (*C.uint64_t)(unsafe.Pointer(&p[0])), nil, C.size_t(len(p)), (*C.uint64_t)(unsafe.Pointer(&point)), nil,
		(*C.uint64_t)(unsafe.Pointer(&res.ClaimedValue)), (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return OpeningProof{}, gmsmErr()
	}
	res.H.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}

// BatchOpenSinglePoint is BatchOpenSinglePoint(polynomials, digests, point, hf, pk, dataTranscript...) (kzg.go:246-339) over
// the resident SRS: the claimed values come from the device (gmsm_poly_eval), the challenge gamma from the package's own
// deriveGamma, and the fold sum_i gamma^i f_i, its quotient by (X - point) and the commitment to it run on the device
// (gmsm_kzg_open_folded). The folded evaluation sum_i gamma^i f_i(point) of kzg.go:287-297 is not formed: the reference
// subtracts it from the constant coefficient, which the division then drops, so H does not depend on it.
func (rk *ResidentProvingKey) BatchOpenSinglePoint(polynomials [][]fr.Element, digests []Digest, point fr.Element, hf hash.Hash, dataTranscript ...[]byte) (BatchOpeningProof, error) {
	if len(digests) != len(polynomials) {
		return BatchOpeningProof{}, ErrInvalidNbDigests
	}
	largestPoly := -1
	for _, p := range polynomials {
		if len(p) == 0 || len(p) > rk.n {
			return BatchOpeningProof{}, ErrInvalidPolynomialSize
		}
		if len(p) > largestPoly {
			largestPoly = len(p)
		}
	}
	if len(polynomials) > 0 && largestPoly < MinDevicePoints && len(rk.host.G1) >= largestPoly {
		return BatchOpenSinglePoint(polynomials, digests, point, hf, rk.host, dataTranscript...)
	}
	if largestPoly < 2 { // Commit of the empty quotient refuses it (kzg.go:326)
		return BatchOpeningProof{}, ErrInvalidPolynomialSize
	}
	lens := make([]C.size_t, len(polynomials))
	total := 0
	for i, p := range polynomials {
		lens[i] = C.size_t(len(p))
		total += len(p)
	}
	flat := make([]fr.Element, 0, total)
	for _, p := range polynomials {
		flat = append(flat, p...)
	}
	var res BatchOpeningProof
	res.ClaimedValues = make([]fr.Element, len(polynomials))
	if rc := C.gmsm_poly_eval(C.GMSM_BN254_G1, (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], C.size_t(len(lens)),
		(*C.uint64_t)(unsafe.Pointer(&point)), nil, (*C.uint64_t)(unsafe.Pointer(&res.ClaimedValues[0]))); rc != 0 {
		return BatchOpeningProof{}, gmsmErr()
	}
	gamma, err := deriveGamma(point, digests, res.ClaimedValues, hf, dataTranscript...)
	if err != nil {
		return BatchOpeningProof{}, err
	}
	var jac bn254.G1Jac
	if rc := C.gmsm_kzg_open_folded(rk.handle, (*C.uint64_t)(unsafe.Pointer(&flat[0])), nil, &lens[0], C.size_t(len(lens)),
		(*C.uint64_t)(unsafe.Pointer(&point)), (*C.uint64_t)(unsafe.Pointer(&gamma)), nil, (*C.uint64_t)(unsafe.Pointer(&jac))); rc != 0 {
		return BatchOpeningProof{}, gmsmErr()
	}
	res.H.FromJacobian(&jac)
	runtime.KeepAlive(rk)
	return res, nil
}

// errNotPowerOfTwo is ToLagrangeG1's error for a length that is not a power of two (utils.go:26-28).
var errNotPowerOfTwo = errors.New("len(coeffs) must be a power of 2")

// ToLagrangeG1Resident is ToLagrangeG1(coeffs) (utils.go:25-64) on the device: the inverse FFT over the points, its
// twiddle products and the batch normalisation run there (gmsm_to_lagrange_g1), with the reference's bits as result.
// coeffs must lie in the r-torsion, as for the reference's mulGLV.
func ToLagrangeG1Resident(coeffs []bn254.G1Affine) ([]bn254.G1Affine, error) {
	if bits.OnesCount64(uint64(len(coeffs))) != 1 {
		return nil, errNotPowerOfTwo
	}
	out := make([]bn254.G1Affine, len(coeffs))
	if rc := C.gmsm_to_lagrange_g1(C.GMSM_BN254_G1, (*C.uint64_t)(unsafe.Pointer(&coeffs[0])), nil, C.size_t(len(coeffs)), nil,
		(*C.uint64_t)(unsafe.Pointer(&out[0])), nil); rc != 0 {
		return nil, gmsmErr()
	}
	return out, nil
}

// ToLagrange returns the Lagrange form of the first size points of the key, ToLagrangeG1(pk.G1[:size]), as a new resident
// key: computed from the points in HBM and registered there (gmsm_bases_to_lagrange) - nothing crosses PCIe. The new key
// has no host copy; Release it (or leave it to the finalizer) like any other.
func (rk *ResidentProvingKey) ToLagrange(size int) (*ResidentProvingKey, error) {
	if size < 0 || size > rk.n {
		return nil, ErrInvalidPolynomialSize
	}
	if bits.OnesCount64(uint64(size)) != 1 {
		return nil, errNotPowerOfTwo
	}
	lk := &ResidentProvingKey{n: size}
	if rc := C.gmsm_bases_to_lagrange(rk.handle, C.size_t(size), &lk.handle); rc != 0 {
		return nil, gmsmErr()
	}
	runtime.SetFinalizer(lk, func(k *ResidentProvingKey) { k.Release() })
	runtime.KeepAlive(rk)
	return lk, nil
}

// Release gives the device memory of the key back (gmsm_bases_release); calls that are still running keep their own reference.
func (rk *ResidentProvingKey) Release() {
	if rk.handle != 0 {
		C.gmsm_bases_release(rk.handle)
		rk.handle = 0
		runtime.SetFinalizer(rk, nil)
	}
}
