// The Fiat-Shamir challenges of package shplonk for packages built on it: fflonk.BatchOpenResident derives gamma and z
// exactly as shplonk.BatchOpen does, over the extended point sets, and deriveChallenge (shplonk.go:278-308) is unexported.
// Compiled in both builds (no tag); uncompiled in the build environment of this repository, like the other Go files.
package shplonk

import (
	"github.com/consensys/gnark-crypto/ecc/bw6-761/fr"
	"github.com/consensys/gnark-crypto/ecc/bw6-761/kzg"
	fiatshamir "github.com/consensys/gnark-crypto/fiat-shamir"
)

// DeriveChallenge is the package's own deriveChallenge: the points, the digests and the extra data are bound to `name`
// in that order, and the challenge is read as an fr.Element.
func DeriveChallenge(name string, points [][]fr.Element, digests []kzg.Digest, t *fiatshamir.Transcript, dataTranscript ...[]byte) (fr.Element, error) {
	return deriveChallenge(name, points, digests, t, dataTranscript...)
}
