//go:build mi355x

// iop.Evaluate on an MI355X. A Go closure cannot run on the device; an Expression of the kind the provers use is a fixed
// sequence of field additions, subtractions and products, the same for every index, so the device form is a Program: built
// once with Input, Const, Point, Add, Sub, Mul and Neg, validated by the library and interpreted by one kernel, one index per
// lane (gmsm_iop_evaluate_expression, include/gmsm.h). Point is w^i with w = fft.Generator(len): the only use gnark's
// numerators make of the closure's argument i; any other function of i goes in as one more input polynomial.
//
// EvaluateDevice keeps Evaluate's checks, texts and result: the form is a label, the size is that of x[0], the shift 0. The
// inputs are read where they are, each through its own layout, size and shift (GetCoeff); r may be the coefficients of an
// input of the same layout and shift 0. Results are the reference's bit for bit.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry point it calls is covered by
// tests/ through the same C ABI, tests/test_iop_expr_abi.py checks tags, package, symbols and arities.
package iop

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr/fft"
)

// Opcodes of a program word (include/gmsm.h, GMSM_EXPR_*): op | dst<<8 | a<<16 | b<<24.
const (
	exprInput = 1 + iota
	exprConst
	exprPoint
	exprAdd
	exprSub
	exprMul
	exprNeg
	exprMaxRegs = 16
)

// Sym is a value of a Program: the result of one instruction.
type Sym int

type exprNode struct {
	op   uint32
	a, b int // symbols for the arithmetic; the input / constant index for Input / Const
}

// Program is the device form of an Expression: a straight-line sequence of field operations, the same for every index.
// Input, Const and Point give symbols, Add, Sub, Mul and Neg combine them; the value of the program is the
// last symbol made.
type Program struct {
	nodes  []exprNode
	consts []fr.Element
}

// NewProgram returns an empty program.
func NewProgram() *Program {
	return &Program{}
}

func (p *Program) push(op uint32, a, b int) Sym {
	p.nodes = append(p.nodes, exprNode{op, a, b})
	return Sym(len(p.nodes) - 1)
}

// Input is x[j].GetCoeff(i).
func (p *Program) Input(j int) Sym {
	return p.push(exprInput, j, 0)
}

// Const is the element v.
func (p *Program) Const(v fr.Element) Sym {
	p.consts = append(p.consts, v)
	return p.push(exprConst, len(p.consts)-1, 0)
}

// Point is w^i, w = fft.Generator(len): what the device offers of the closure's argument i.
func (p *Program) Point() Sym {
	return p.push(exprPoint, 0, 0)
}

// Add is a + b.
func (p *Program) Add(a, b Sym) Sym {
	return p.push(exprAdd, int(a), int(b))
}

// Sub is a - b.
func (p *Program) Sub(a, b Sym) Sym {
	return p.push(exprSub, int(a), int(b))
}

// Mul is a * b.
func (p *Program) Mul(a, b Sym) Sym {
	return p.push(exprMul, int(a), int(b))
}

// Neg is -a.
func (p *Program) Neg(a Sym) Sym {
	return p.push(exprNeg, int(a), int(a))
}

func (n exprNode) operands() []int {
	switch n.op {
	case exprAdd, exprSub, exprMul:
		return []int{n.a, n.b}
	case exprNeg:
		return []int{n.a}
	}
	return nil
}

// words gives the instructions in the order they were made, with registers allocated by liveness: a register is free again
// after the last use of its symbol. The value of the program is the last symbol made.
func (p *Program) words() ([]uint32, bool, error) {
	if len(p.nodes) == 0 {
		return nil, false, errors.New("gmsm: empty program")
	}
	lastUse := make([]int, len(p.nodes))
	for k, n := range p.nodes {
		lastUse[k] = k
		for _, o := range n.operands() {
			if o < 0 || o >= k {
				return nil, false, errors.New("gmsm: a symbol of another program")
			}
			lastUse[o] = k
		}
	}
	reg := make([]int, len(p.nodes))
	var busy [exprMaxRegs]bool
	words := make([]uint32, 0, len(p.nodes))
	hasPoint := false
	for k, n := range p.nodes {
		a, b := uint32(n.a), uint32(0)
		ops := n.operands()
		if len(ops) > 0 {
			a = uint32(reg[ops[0]])
		}
		if len(ops) > 1 {
			b = uint32(reg[ops[1]])
		}
		for _, o := range ops { // the destination may be an operand's register: the lane reads both before it writes
			if lastUse[o] == k {
				busy[reg[o]] = false
			}
		}
		r := 0
		for r < exprMaxRegs && busy[r] {
			r++
		}
		if r == exprMaxRegs {
			return nil, false, errors.New("gmsm: more than 16 registers are live at once")
		}
		if lastUse[k] != k || k == len(p.nodes)-1 {
			busy[r] = true
		}
		reg[k] = r
		hasPoint = hasPoint || n.op == exprPoint
		words = append(words, n.op|uint32(r)<<8|a<<16|b<<24)
	}
	return words, hasPoint, nil
}

// EvaluateDevice is Evaluate for a Program, on the device.
func EvaluateDevice(p *Program, r []fr.Element, form Form, x ...*Polynomial) (*Polynomial, error) {
	if len(x) == 0 {
		return nil, errors.New("need at lest one input")
	}
	n := x[0].coefficients.Len()
	m := len(x)
	for i := 1; i < m; i++ {
		if n != x[i].coefficients.Len() {
			return nil, ErrInconsistentSize
		}
	}
	if r == nil {
		r = make([]fr.Element, n)
	} else if len(r) != n {
		return nil, ErrInconsistentSize
	}
	words, hasPoint, err := p.words()
	if err != nil {
		return nil, err
	}
	if n > 0 {
		var domain C.uint64_t
		if hasPoint {
			if domain, err = gmsmDomain(fft.NewDomain(uint64(n))); err != nil {
				return nil, err
			}
		}
		// the array of input pointers holds Go pointers: they are pinned for the duration of the call
		var pinner runtime.Pinner
		defer pinner.Unpin()
		polys := make([]*C.uint64_t, m)
		sizes := make([]C.size_t, m)
		shifts := make([]C.int64_t, m)
		layouts := make([]C.uint32_t, m)
		for j, pj := range x {
			pinner.Pin(&(*pj.coefficients)[0])
			polys[j] = gmsmElems(*pj.coefficients)
			sizes[j], shifts[j], layouts[j] = C.size_t(pj.size), C.int64_t(pj.shift), C.uint32_t(pj.Layout)
		}
		var consts *C.uint64_t
		if len(p.consts) > 0 {
			consts = gmsmElems(p.consts)
		}
		if rc := C.gmsm_iop_evaluate_expression(gmsmG1, domain, (*C.uint32_t)(unsafe.Pointer(&words[0])), C.size_t(len(words)), consts, C.size_t(len(p.consts)), (**C.uint64_t)(unsafe.Pointer(&polys[0])), nil, C.size_t(m), C.size_t(n), &sizes[0], &shifts[0], &layouts[0], C.int(form.Layout), nil, gmsmElems(r), nil); rc != 0 {
			return nil, gmsmErr()
		}
	}
	res := NewPolynomial(&r, form)
	res.size = x[0].size
	res.shift = 0
	return res, nil
}
