"""cwfa_amd -- MI355X-native implementation of CWFA's inverse (reconstruction) / forward-NLL hot path.

Python mirrors of the reference's modules (``FrEIA``, ``INN_utils``, ``networks``, ``unet``, hot-path part of ``CWFA``)
over hand-written HIP kernels in ``libcwfa_hip.so`` (C ABI: include/cwfa_hip.h).  There is no CPU or PyTorch fallback:
ops raise on non-HIP tensors and on a missing extension.

    import cwfa_amd; cwfa_amd.install()     # then the reference's main.py imports resolve to this package
    cwfa_amd.install(precision="fp16")      # ... for its default --use_half_precision 1 (autocast)
    cwfa_amd.install(lion=True)             # ... and `from lion_pytorch import Lion` resolves to cwfa_amd.optim.Lion
    cwfa_amd.install(losses=True)           # ... and `import losses as Losses` resolves to cwfa_amd.losses (the fused wL2 loss)
    cwfa_amd.install(utils=True)            # ... and `from utils import *` resolves to cwfa_amd.utils (XLFMDeconv, load_PSF_OTF, ...)
"""
import sys

__version__ = "0.1.0"


def install(precision=None, lion=False, losses=False, utils=False):
    """Register this package's modules under the reference's top-level import names (FrEIA, INN_utils, networks, unet)
    so that code written against the reference (``import FrEIA.framework as Ff``, ``from networks import *``) runs on
    the HIP implementation unchanged.  Call before importing the reference's driver.

    ``precision``: None leaves the arithmetic as it is; a mode name ("fp32", "split_bf16", "bf16", "fp16") is passed to
    ``ops.set_precision``.  "fp16" is the arithmetic of the reference's default ``--use_half_precision 1`` (CUDA autocast:
    fp16 operands, fp32 accumulation); the installed modules compute the same inside and outside an autocast region.

    ``lion``: True also registers a module ``lion_pytorch`` whose ``Lion`` is ``cwfa_amd.optim.Lion`` (the fused HIP step), so that
    the reference's ``from lion_pytorch import Lion`` and its ``opt_to_use=Lion`` default (CWFA.py:24,381) resolve to it.  With the
    default False nothing is registered under that name.

    ``losses``: True also registers ``cwfa_amd.losses`` under the name ``losses``, so that the reference's ``import losses as Losses``
    (CWFA.py:27) and its ``Losses.weighted_mse_loss(curr_gt, upsampled_vol)`` calls (the `wL2` loss) run the fused HIP pass.  That
    module holds only what CWFA.py uses from losses.py.  With the default False nothing is registered under that name.

    ``utils``: True also registers ``cwfa_amd.utils`` under the name ``utils``, so that the ``from utils import *`` of the reference's
    ``main_deconvolve_dataset.py`` finds ``XLFMDeconv``, ``load_PSF_OTF``, ``fft_conv_split`` and the other mirrors of that module
    (DESIGN.md section 17).  The module holds no file readers (the reference's ``utils`` re-exports its dataset classes); with the
    default False nothing is registered under that name."""
    from . import FrEIA, INN_utils, networks, unet
    if precision is not None:
        from . import ops
        ops.set_precision(precision)
    sys.modules["FrEIA"] = FrEIA
    sys.modules["FrEIA.framework"] = FrEIA.framework
    sys.modules["FrEIA.modules"] = FrEIA.modules
    sys.modules["INN_utils"] = INN_utils
    sys.modules["networks"] = networks
    sys.modules["unet"] = unet
    if lion:
        import types
        from . import optim
        mod = types.ModuleType("lion_pytorch", "cwfa_amd.optim.Lion under the name the reference imports it by")
        mod.Lion = optim.Lion
        mod.__all__ = ["Lion"]
        sys.modules["lion_pytorch"] = mod
    if losses:
        from . import losses as losses_mod
        sys.modules["losses"] = losses_mod
    if utils:
        from . import utils as utils_mod
        sys.modules["utils"] = utils_mod
    return FrEIA, INN_utils, networks, unet
