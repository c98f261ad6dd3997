//go:build mi355x

// gkr.Prove on an MI355X. The sumcheck of every wire runs over a device claim (gmsm_gkr_claim_new / _next / _final,
// include/gmsm.h): the eq table and copies of the gate's input assignments stay in HBM between the rounds, each round is one
// pass that folds them and evaluates the gate at Degree() + 1 points per instance, and the Fiat-Shamir transcript stays here.
// A Gate is a Go closure, which cannot run on the device: a DeviceGate also emits itself into an iop.Program, the
// straight-line form that iop.EvaluateDevice uses. The five named gates do; a circuit with another kind of gate is refused.
//
// ProveDevice keeps Prove's setup, claims manager, challenge names, base challenges and proof layout: the proof is the
// reference's, element for element. The memory Pool has no counterpart on the device; WithPool is accepted and unused by
// the claims.
//
// NOT compiled in the build environment of this repository (no Go toolchain there); the C entry points it calls are covered
// by tests/ through the same C ABI, tests/test_gkr_abi.py checks tags, package, symbols and arities.
package gkr

/*
#cgo CFLAGS: -I${SRCDIR}/../../../../third_party/gmsm/include
#cgo LDFLAGS: -L${SRCDIR}/../../../../third_party/gmsm/lib -lgmsm -Wl,-rpath,${SRCDIR}/../../../../third_party/gmsm/lib
#include "gmsm.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"strconv"
	"unsafe"

	"github.com/consensys/gnark-crypto/ecc/bn254/fr"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/iop"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/polynomial"
	"github.com/consensys/gnark-crypto/ecc/bn254/fr/sumcheck"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

const gmsmG1 = C.int(C.GMSM_BN254_G1)

func gmsmErr() error { return errors.New("gmsm: " + C.GoString(C.gmsm_last_error())) }

func gmsmElems(v []fr.Element) *C.uint64_t { return (*C.uint64_t)(unsafe.Pointer(&v[0])) }

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

// gateProgram is the gate of a wire as instruction words over nbIn inputs.
func gateProgram(g DeviceGate, nbIn int) ([]uint32, []fr.Element, error) {
	p := iop.NewProgram()
	in := make([]iop.Sym, nbIn)
	for j := range in {
		in[j] = p.Input(j)
	}
	return p.Words(g.Emit(p, in))
}

// deviceClaims is eqTimesGateEvalSumcheckClaims over a claim handle: sumcheck.Claims for sumcheck.Prove.
type deviceClaims struct {
	lazy   *eqTimesGateEvalSumcheckLazyClaims
	words  []uint32
	consts []fr.Element
	handle C.uint64_t
	live   bool
	err    error // the first failure of a device call; the polynomials after it are zero and the proof is discarded
}

func (c *deviceClaims) VarsNum() int { return len(c.lazy.evaluationPoints[0]) }

func (c *deviceClaims) ClaimsNum() int { return len(c.lazy.claimedEvaluations) }

// inputs are the wires whose assignments the gate reads: the wire itself for an input wire (identity gate).
func (c *deviceClaims) inputs() []*Wire {
	if c.lazy.wire.IsInput() {
		return []*Wire{c.lazy.wire}
	}
	return c.lazy.wire.Inputs
}

func (c *deviceClaims) fail() {
	if c.err == nil {
		c.err = gmsmErr()
	}
}

func (c *deviceClaims) Combine(combinationCoeff fr.Element) polynomial.Polynomial {
	ins := c.inputs()
	nbVars := c.VarsNum()
	gJ := make(polynomial.Polynomial, c.lazy.wire.Gate.Degree()+1)
	// the array of table pointers holds Go pointers: they are pinned for the duration of the call (the library copies the tables)
	var pinner runtime.Pinner
	defer pinner.Unpin()
	tables := make([]*C.uint64_t, len(ins))
	for j, in := range ins {
		t := c.lazy.manager.assignment[in]
		pinner.Pin(&t[0])
		tables[j] = gmsmElems(t)
	}
	points := make([]fr.Element, 0, len(c.lazy.evaluationPoints)*nbVars)
	for _, pt := range c.lazy.evaluationPoints {
		points = append(points, pt...)
	}
	var consts *C.uint64_t
	if len(c.consts) > 0 {
		consts = gmsmElems(c.consts)
	}
	comb := []fr.Element{combinationCoeff}
	if rc := C.gmsm_gkr_claim_new(gmsmG1, (*C.uint32_t)(unsafe.Pointer(&c.words[0])), C.size_t(len(c.words)), consts, C.size_t(len(c.consts)), C.size_t(c.lazy.wire.Gate.Degree()), (**C.uint64_t)(unsafe.Pointer(&tables[0])), nil, C.size_t(len(ins)), C.size_t(1)<<nbVars, gmsmElems(points), C.size_t(len(c.lazy.evaluationPoints)), gmsmElems(comb), nil, gmsmElems(gJ), &c.handle); rc != 0 {
		c.fail()
		return gJ
	}
	c.live = true
	return gJ
}

func (c *deviceClaims) Next(element fr.Element) polynomial.Polynomial {
	gJ := make(polynomial.Polynomial, c.lazy.wire.Gate.Degree()+1)
	r := []fr.Element{element}
	if !c.live {
		return gJ
	}
	if rc := C.gmsm_gkr_claim_next(c.handle, gmsmElems(r), gmsmElems(gJ)); rc != 0 {
		c.fail()
	}
	return gJ
}

func (c *deviceClaims) ProveFinalEval(r []fr.Element) interface{} {
	wire := c.lazy.wire
	folded := make([]fr.Element, len(c.inputs()))
	if c.live {
		if rc := C.gmsm_gkr_claim_final(c.handle, gmsmElems(r[len(r)-1:]), gmsmElems(folded)); rc != 0 {
			c.fail()
		}
	}
	// defer the proof, return list of claims: the first occurrence of each distinct input wire, never the wire itself
	evaluations := make([]fr.Element, 0, len(wire.Inputs))
	noMoreClaimsAllowed := make(map[*Wire]struct{}, len(wire.Inputs))
	noMoreClaimsAllowed[wire] = struct{}{}
	for inI, in := range wire.Inputs {
		if _, found := noMoreClaimsAllowed[in]; !found {
			noMoreClaimsAllowed[in] = struct{}{}
			c.lazy.manager.add(in, r, folded[inI])
			evaluations = append(evaluations, folded[inI])
		}
	}
	return evaluations
}

func (c *deviceClaims) release() {
	if c.live {
		C.gmsm_gkr_claim_release(c.handle)
		c.live = false
	}
}

// ProveDevice is Prove with every sumcheck on the device.
func ProveDevice(c Circuit, assignment WireAssignment, transcriptSettings fiatshamir.Settings, options ...Option) (Proof, error) {
	o, err := setup(c, assignment, transcriptSettings, options...)
	if err != nil {
		return nil, err
	}
	defer o.workers.Stop()

	// every gate that will be proven needs its device form, before any work
	type program struct {
		words  []uint32
		consts []fr.Element
	}
	programs := make(map[*Wire]program, len(c))
	for _, wire := range o.sorted {
		if wire.noProof() {
			continue
		}
		g, ok := wire.Gate.(DeviceGate)
		if !ok {
			return nil, errors.New("gmsm: a gate of the circuit is no DeviceGate")
		}
		nbIn := len(wire.Inputs)
		if nbIn == 0 {
			nbIn = 1
		}
		var pr program
		if pr.words, pr.consts, err = gateProgram(g, nbIn); err != nil {
			return nil, err
		}
		programs[wire] = pr
	}

	claims := newClaimsManager(c, assignment, o)

	proof := make(Proof, len(c))
	// firstChallenge called rho in the paper
	var firstChallenge []fr.Element
	firstChallenge, err = getChallenges(o.transcript, getFirstChallengeNames(o.nbVars, o.transcriptPrefix))
	if err != nil {
		return nil, err
	}

	wirePrefix := o.transcriptPrefix + "w"
	var baseChallenge [][]byte
	for i := len(c) - 1; i >= 0; i-- {

		wire := o.sorted[i]

		if wire.IsOutput() {
			claims.add(wire, firstChallenge, assignment[wire].Evaluate(firstChallenge, claims.memPool))
		}

		if wire.noProof() { // input wires with one claim only
			proof[i] = sumcheck.Proof{
				PartialSumPolys: []polynomial.Polynomial{},
				FinalEvalProof:  []fr.Element{},
			}
		} else {
			claim := &deviceClaims{lazy: claims.getLazyClaim(wire), words: programs[wire].words, consts: programs[wire].consts}
			proof[i], err = sumcheck.Prove(
				claim, fiatshamir.WithTranscript(o.transcript, wirePrefix+strconv.Itoa(i)+".", baseChallenge...),
			)
			claim.release()
			if err == nil {
				err = claim.err
			}
			if err != nil {
				return nil, err
			}

			finalEvalProof := proof[i].FinalEvalProof.([]fr.Element)
			baseChallenge = make([][]byte, len(finalEvalProof))
			for j := range finalEvalProof {
				bytes := finalEvalProof[j].Bytes()
				baseChallenge[j] = bytes[:]
			}
		}
		// the verifier checks a single claim about input wires itself
		claims.deleteClaim(wire)
	}

	return proof, nil
}
