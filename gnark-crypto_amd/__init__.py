"""MI355X-native multi-scalar multiplication for gnark-crypto's ecc/<curve>.MultiExp path.

Import with importlib (the directory name carries a hyphen):
    gm = importlib.import_module("gnark-crypto_amd")
"""
from .curves import BLS12_381, BN254, BW6_761, CURVES  # noqa: F401
from .multiexp import G1Affine, G1Jac, G2Affine, G2Jac, MultiExpConfig, get_devices, set_devices  # noqa: F401
from ._lib import options, set_option, get_option, trim, shutdown  # noqa: F401  (gmsm_set_option / gmsm_trim / gmsm_shutdown)
from . import fft  # noqa: F401  (fr/fft mirror: fft.NewDomain, fft.DIT / fft.DIF, fft.OnCoset, fft.BitReverse)
from . import kzg  # noqa: F401  (kzg mirror: kzg.Open, kzg.BatchOpenSinglePoint, kzg.PolyEval, kzg.DividePolyByXMinusA, kzg.ToLagrangeG1)
from . import shplonk  # noqa: F401  (shplonk mirror: shplonk.BatchOpen, shplonk.OpenW, shplonk.OpenWPrime)
from . import fflonk  # noqa: F401  (fflonk mirror: fflonk.Fold, fflonk.FoldAndCommit, fflonk.BatchOpen, fflonk.OpenW, fflonk.OpenWPrime)
from . import iop  # noqa: F401  (fr/iop mirror: iop.BuildRatioCopyConstraint, iop.BuildRatioShuffledVectors; fr.BatchInvert as iop.BatchInvert; iop.Polynomial with its basis changes and Evaluate, iop.DivideByXMinusOne, iop.Evaluate over iop.Program)
from . import mpcsetup  # noqa: F401  (mpcsetup mirror: mpcsetup.UpdateMonomialsG1/G2, mpcsetup.ScaleG1/G2, mpcsetup.BatchScaleG1/G2, mpcsetup.linearCombinationsG1/G2)
from . import polynomial  # noqa: F401  (fr/polynomial mirror: polynomial.MultiLin with Fold, Evaluate, Eq; polynomial.EvalEq)
from . import fiatshamir  # noqa: F401  (fiat-shamir mirror: fiatshamir.Transcript, NewTranscript, Bind, ComputeChallenge; host only)
from . import sumcheck  # noqa: F401  (fr/sumcheck mirror: sumcheck.Prove over a claims object)
from . import gkr  # noqa: F401  (fr/gkr mirror: gkr.Gate, gkr.Gates, gkr.Wire, gkr.Circuit, gkr.WireAssignment.Complete, gkr.Prove; gkr.Claim is the device handle of one wire's sumcheck claim)
from . import mimc  # noqa: F401  (fr/mimc mirror: mimc.NewMiMC with Write / Sum / Reset / State / SetState, mimc.Sum, mimc.GetConstants; mimc.SumBatch hashes many messages on the device)
from . import merkletree  # noqa: F401  (accumulator/merkletree mirror over MiMC: merkletree.DeviceTree with Root and Prove, merkletree.VerifyProof on the host)
from . import fri  # noqa: F401  (fr/fri mirror: fri.RADIX_2_FRI.New with BuildProofOfProximity / VerifyProofOfProximity / Open / VerifyOpening; fri.Oracle is the device handle of the committed layers and their trees)
