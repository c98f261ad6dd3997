//go:build !mi355x

// The same API as gkr_mi355x.go without the device: a DeviceGate still emits itself into an iop.Program, and ProveDevice is
// the package's own Prove, so callers compile under either tag and a build without it computes what the reference computes.
package gkr

import (
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/iop"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

// DeviceGate is a Gate that can write itself as a straight-line program: Emit makes the gate's value out of the symbols
// of its inputs with p.Add, p.Sub, p.Mul, p.Neg and p.Const, and returns the last symbol it made, or one of the inputs.
type DeviceGate interface {
	Gate
	Emit(p *iop.Program, in []iop.Sym) iop.Sym
}

func (IdentityGate) Emit(p *iop.Program, in []iop.Sym) iop.Sym {
	return in[0]
}

func (g AddGate) Emit(p *iop.Program, in []iop.Sym) iop.Sym {
	res := in[0]
	for i := 1; i < len(in); i++ {
		res = p.Add(res, in[i])
	}
	return res
}

func (g MulGate) Emit(p *iop.Program, in []iop.Sym) iop.Sym {
	res := in[0]
	for i := 1; i < len(in); i++ {
		res = p.Mul(res, in[i])
	}
	return res
}

func (g SubGate) Emit(p *iop.Program, in []iop.Sym) iop.Sym {
	return p.Sub(in[0], in[1])
}

func (g NegGate) Emit(p *iop.Program, in []iop.Sym) iop.Sym {
	return p.Neg(in[0])
}

// ProveDevice is Prove.
func ProveDevice(c Circuit, assignment WireAssignment, transcriptSettings fiatshamir.Settings, options ...Option) (Proof, error) {
	return Prove(c, assignment, transcriptSettings, options...)
}
