//go:build !mi355x

// The same API as polynomial_mi355x.go without the device: calls into the package's own methods, so a build without the tag
// behaves exactly like the reference.
package iop

import (
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr/fft"
)

// ToLagrangeDevice is ToLagrange.
func (p *Polynomial) ToLagrangeDevice(d *fft.Domain) *Polynomial {
	return p.ToLagrange(d)
}

// ToCanonicalDevice is ToCanonical.
func (p *Polynomial) ToCanonicalDevice(d *fft.Domain) *Polynomial {
	return p.ToCanonical(d)
}

// ToLagrangeCosetDevice is ToLagrangeCoset.
func (p *Polynomial) ToLagrangeCosetDevice(d *fft.Domain) *Polynomial {
	return p.ToLagrangeCoset(d)
}

// EvaluateDevice is Evaluate.
func (p *Polynomial) EvaluateDevice(x fr.Element) fr.Element {
	return p.Evaluate(x)
}

// DivideByXMinusOneDevice is DivideByXMinusOne.
func DivideByXMinusOneDevice(a *Polynomial, domains [2]*fft.Domain) (*Polynomial, error) {
	return DivideByXMinusOne(a, domains)
}
