"""HyperSeg on the AMD Instinct MI355X: PyTorch-ROCm modules over hand-written HIP kernels."""


def __getattr__(name):
    # exported lazily: importing the package must not import torch-heavy submodules (or the HIP library) as a side effect
    if name == 'InputNorm':
        from .utils.inference import InputNorm
        return InputNorm
    if name == 'FrameResize':
        from .utils.inference import FrameResize
        return FrameResize
    if name == 'ColorJitterParams':
        from .utils.jitter import ColorJitterParams
        return ColorJitterParams
    if name == 'GaussianBlurParams':
        from .utils.blur import GaussianBlurParams
        return GaussianBlurParams
    if name == 'Overlay':
        from .utils.inference import Overlay
        return Overlay
    if name == 'Confidence':
        from .utils.confidence import Confidence
        return Confidence
    if name == 'LabelCodec':
        from .utils.labels import LabelCodec
        return LabelCodec
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
