//go:build !mi355x

// The API of mimc_mi355x.go for builds without the tag: one NewMiMC() per message - callers compile either way and nothing
// of the reference changes.
package mimc

import (
	"errors"

	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
)

// ErrBatchShape is returned when the elements do not divide into messages of msgLen elements.
var ErrBatchShape = errors.New("mimc: msgLen must be positive and divide the number of elements")

// SumBatchDevice hashes len(msgs)/msgLen messages of msgLen elements each with NewMiMC() (mimc.go:57-163).
func SumBatchDevice(msgs []fr.Element, msgLen int) ([]fr.Element, error) {
	if msgLen <= 0 || len(msgs)%msgLen != 0 {
		return nil, ErrBatchShape
	}
	res := make([]fr.Element, len(msgs)/msgLen)
	for i := range res {
		h := NewMiMC()
		for _, e := range msgs[i*msgLen : (i+1)*msgLen] {
			b := e.Bytes()
			if _, err := h.Write(b[:]); err != nil {
				return nil, err
			}
		}
		res[i].SetBytes(h.Sum(nil))
	}
	return res, nil
}
