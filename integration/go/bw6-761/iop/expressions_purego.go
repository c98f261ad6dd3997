//go:build !mi355x

// The same API as expressions_mi355x.go without the device: the Program is interpreted on the host with fr.Element methods
// and handed to the package's own Evaluate, so callers compile under either tag and a build without it computes what the
// reference computes.
package iop

import (
	"errors"
	"math/big"

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

// EvaluateDevice is Evaluate over the Expression that interprets p.
func EvaluateDevice(p *Program, r []fr.Element, form Form, x ...*Polynomial) (*Polynomial, error) {
	if len(x) == 0 {
		return nil, errors.New("need at lest one input")
	}
	words, hasPoint, err := p.words()
	if err != nil {
		return nil, err
	}
	for _, n := range p.nodes {
		if n.op == exprInput && (n.a < 0 || n.a >= len(x)) {
			return nil, errors.New("gmsm: the program reads an input that was not given")
		}
	}
	var w fr.Element
	if hasPoint {
		w.Set(&fft.NewDomain(uint64(x[0].coefficients.Len())).Generator)
	}
	f := func(i int, vx ...fr.Element) fr.Element {
		var reg [exprMaxRegs]fr.Element
		var last fr.Element
		for _, ins := range words {
			op, dst, a, b := ins&0xff, (ins>>8)&0xff, (ins>>16)&0xff, ins>>24
			switch op {
			case exprInput:
				last.Set(&vx[a])
			case exprConst:
				last.Set(&p.consts[a])
			case exprPoint:
				last.Exp(w, big.NewInt(int64(i)))
			case exprAdd:
				last.Add(&reg[a], &reg[b])
			case exprSub:
				last.Sub(&reg[a], &reg[b])
			case exprMul:
				last.Mul(&reg[a], &reg[b])
			case exprNeg:
				last.Neg(&reg[a])
			}
			reg[dst].Set(&last)
		}
		return last
	}
	return Evaluate(f, r, form, x...)
}
