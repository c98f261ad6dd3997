//go:build mi355x

// accumulator/merkletree over MiMC, built on an MI355X: every leaf's sum and every level above them in one pass over HBM
// (gmsm_merkle_new), all proofs of a query in one gather launch (gmsm_merkle_prove). The tree is the one merkletree.New(NewMiMC())
// builds from the leaves' bytes - leafSum(data) = H(data), nodeSum(a, b) = H(a || b), RFC 6962's shape - so roots and proof sets
// are the reference's bit for bit and merkletree.VerifyProof accepts them unchanged.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_mimc_stubs.py checks tags, package, symbols and arities.
package mimc

/*
#include "gmsm.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
)

// DeviceTree is a Merkle tree resident on the device: its levels and its leaves' data stay in HBM until Release.
type DeviceTree struct {
	handle  C.uint64_t
	n       int
	leafLen int
	depth   int
}

// NewDeviceTree builds the tree over len(leaves)/leafLen leaves of leafLen elements each; a leaf's data is the concatenation
// of its elements' Bytes().
func NewDeviceTree(leaves []fr.Element, leafLen int) (*DeviceTree, error) {
	if leafLen <= 0 || len(leaves) == 0 || len(leaves)%leafLen != 0 {
		return nil, ErrBatchShape
	}
	t := &DeviceTree{n: len(leaves) / leafLen, leafLen: leafLen}
	if rc := C.gmsm_merkle_new(gmsmG1, (*C.uint64_t)(unsafe.Pointer(&leaves[0])), nil, C.size_t(t.n), C.size_t(leafLen), 1, nil, &t.handle); rc != 0 {
		return nil, gmsmErr()
	}
	var depth C.uint
	if rc := C.gmsm_merkle_info(t.handle, nil, nil, &depth); rc != 0 {
		return nil, gmsmErr()
	}
	t.depth = int(depth)
	runtime.SetFinalizer(t, func(t *DeviceTree) { _ = t.Release() })
	return t, nil
}

// NumLeaves returns the number of leaves.
func (t *DeviceTree) NumLeaves() uint64 { return uint64(t.n) }

// Root returns the Merkle root, as (*merkletree.Tree).Root does.
func (t *DeviceTree) Root() ([]byte, error) {
	var root fr.Element
	if rc := C.gmsm_merkle_root(t.handle, (*C.uint64_t)(unsafe.Pointer(&root))); rc != 0 {
		return nil, gmsmErr()
	}
	b := root.Bytes()
	return b[:], nil
}

// Prove returns one proof set per index, as (*merkletree.Tree).Prove returns it after SetIndex(index) and a Push of every leaf:
// the leaf's data, then the siblings' sums bottom up.
func (t *DeviceTree) Prove(indices []uint64) ([][][]byte, error) {
	k := len(indices)
	if k == 0 {
		return nil, nil
	}
	leaves := make([]fr.Element, k*t.leafLen)
	siblings := make([]fr.Element, k*t.depth+1)
	counts := make([]C.uint32_t, k)
	if rc := C.gmsm_merkle_prove(t.handle, (*C.uint64_t)(unsafe.Pointer(&indices[0])), C.size_t(k), (*C.uint64_t)(unsafe.Pointer(&leaves[0])),
		(*C.uint64_t)(unsafe.Pointer(&siblings[0])), &counts[0]); rc != 0 {
		return nil, gmsmErr()
	}
	res := make([][][]byte, k)
	for j := range res {
		data := make([]byte, 0, t.leafLen*fr.Bytes)
		for _, e := range leaves[j*t.leafLen : (j+1)*t.leafLen] {
			b := e.Bytes()
			data = append(data, b[:]...)
		}
		res[j] = append(res[j], data)
		for _, e := range siblings[j*t.depth : j*t.depth+int(counts[j])] {
			b := e.Bytes()
			res[j] = append(res[j], b[:])
		}
	}
	runtime.KeepAlive(t)
	return res, nil
}

// Release frees the tree's device memory; the tree must not be used afterwards.
func (t *DeviceTree) Release() error {
	if t.handle == 0 {
		return nil
	}
	rc := C.gmsm_merkle_release(t.handle)
	t.handle = 0
	runtime.SetFinalizer(t, nil)
	if rc != 0 {
		return gmsmErr()
	}
	return nil
}
