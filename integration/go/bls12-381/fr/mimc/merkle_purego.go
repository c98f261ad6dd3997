//go:build !mi355x

// The API of merkle_mi355x.go for builds without the tag: merkletree.New(NewMiMC()) over the leaves' bytes, one pass per
// proof - callers compile either way and nothing of the reference changes.
package mimc

import (
	"github.com/consensys/gnark-crypto/accumulator/merkletree"
	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
)

// DeviceTree keeps the leaves' data; every Root and Prove pushes them through a merkletree.Tree.
type DeviceTree struct {
	leaves [][]byte
}

// NewDeviceTree takes len(leaves)/leafLen leaves of leafLen elements each; a leaf's data is the concatenation of its elements'
// Bytes().
func NewDeviceTree(leaves []fr.Element, leafLen int) (*DeviceTree, error) {
	if leafLen <= 0 || len(leaves) == 0 || len(leaves)%leafLen != 0 {
		return nil, ErrBatchShape
	}
	t := &DeviceTree{leaves: make([][]byte, len(leaves)/leafLen)}
	for i := range t.leaves {
		for _, e := range leaves[i*leafLen : (i+1)*leafLen] {
			b := e.Bytes()
			t.leaves[i] = append(t.leaves[i], b[:]...)
		}
	}
	return t, nil
}

// NumLeaves returns the number of leaves.
func (t *DeviceTree) NumLeaves() uint64 { return uint64(len(t.leaves)) }

// Root returns the Merkle root (tree.go:299-314).
func (t *DeviceTree) Root() ([]byte, error) {
	tree := merkletree.New(NewMiMC())
	for _, d := range t.leaves {
		tree.Push(d)
	}
	return tree.Root(), nil
}

// Prove returns one proof set per index (tree.go:137-199).
func (t *DeviceTree) Prove(indices []uint64) ([][][]byte, error) {
	res := make([][][]byte, len(indices))
	for j, index := range indices {
		tree := merkletree.New(NewMiMC())
		if err := tree.SetIndex(index); err != nil {
			return nil, err
		}
		for _, d := range t.leaves {
			tree.Push(d)
		}
		_, res[j], _, _ = tree.Prove()
	}
	return res, nil
}

// Release drops the leaves.
func (t *DeviceTree) Release() error {
	t.leaves = nil
	return nil
}
