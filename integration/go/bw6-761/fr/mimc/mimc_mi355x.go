//go:build mi355x

// Many independent MiMC hashes of package fr/mimc on an MI355X. One hash is a chain of three dependent products per round
// and block (mimc.go:130-163), which a CPU walks one after the other; gmsm_mimc_sum_batch gives every message a lane of its
// own. Digests are the reference's bit for bit: each is a uniquely determined canonical element.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_go_mimc_stubs.py checks tags, package, symbols and arities.
package mimc

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
)

const gmsmG1 = C.int(C.GMSM_BW6_761_G1)

// ErrBatchShape is returned when the elements do not divide into messages of msgLen elements.
var ErrBatchShape = errors.New("mimc: msgLen must be positive and divide the number of elements")

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

// SumBatchDevice hashes len(msgs)/msgLen messages of msgLen elements each, message i being msgs[i*msgLen:(i+1)*msgLen]:
// what NewMiMC() returns for each after Write of the elements' Bytes() and Sum, as elements.
func SumBatchDevice(msgs []fr.Element, msgLen int) ([]fr.Element, error) {
	if msgLen <= 0 || len(msgs)%msgLen != 0 {
		return nil, ErrBatchShape
	}
	count := len(msgs) / msgLen
	res := make([]fr.Element, count)
	if count == 0 {
		return res, nil
	}
	if rc := C.gmsm_mimc_sum_batch(gmsmG1, (*C.uint64_t)(unsafe.Pointer(&msgs[0])), nil, C.size_t(count), C.size_t(msgLen), C.size_t(msgLen),
		nil, nil, (*C.uint64_t)(unsafe.Pointer(&res[0])), nil); rc != 0 {
		return nil, gmsmErr()
	}
	return res, nil
}
