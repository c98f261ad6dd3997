// A Program's instruction words for callers outside this package (fr/gkr: a gate is such a program, include/gmsm.h
// gmsm_gkr_claim_new). No build tag and no C: both builds of expressions_*.go have the Program and its words.
package iop

import (
	"errors"

	"github.com/consensys/gnark-crypto/ecc/bls12-381/fr"
)

// Words gives the program whose value is result: its instruction words (op | dst<<8 | a<<16 | b<<24) and its constants.
// The value of a program is the last symbol made, so result must be that symbol, or an Input - which is then made once
// more, as the last one. A program with Point is refused: only an expression over a domain has an index.
func (p *Program) Words(result Sym) ([]uint32, []fr.Element, error) {
	if int(result) != len(p.nodes)-1 {
		if result < 0 || int(result) >= len(p.nodes) || p.nodes[result].op != exprInput {
			return nil, nil, errors.New("gmsm: the result must be the last symbol made, or an input")
		}
		p.Input(p.nodes[result].a)
	}
	words, hasPoint, err := p.words()
	if err != nil {
		return nil, nil, err
	}
	if hasPoint {
		return nil, nil, errors.New("gmsm: a program with Point has no words outside an evaluation over a domain")
	}
	return words, p.consts, nil
}
