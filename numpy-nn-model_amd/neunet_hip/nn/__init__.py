"""neunet_hip.nn -- the names user code takes from `neunet.nn`, bound to the HIP implementations for the
dense hot path (Linear, Conv2d, ReLU, Swish, Softmax, RMSNorm, CrossEntropyLoss)."""
from .modules import Module, ModuleList, Sequential  # noqa: F401
from .parameter import Parameter  # noqa: F401
from . import experimental  # noqa: F401
from . import utils  # noqa: F401  (clip_grad_norm_, get_grad_norm)
from .experimental import (HIPConv2d as Conv2d, HIPCrossEntropyLoss, HIPLinear as Linear,  # noqa: F401
                           HIPLinearSwish as LinearSwish, HIPReLU as ReLU, HIPRMSNorm as RMSNorm,
                           HIPSoftmax as Softmax, HIPSwish as Swish, HIPFusedSwishAndMul as FusedSwishAndMul,
                           HIPEmbedding as Embedding, HIPDropout as Dropout, HIPMultiHeadAttention as MultiHeadAttention,
                           HIPPositionalEncoding as PositionalEncoding, HIPBatchNorm2d as BatchNorm2d,
                           HIPLeakyReLU as LeakyReLU, HIPMaxPool2d as MaxPool2d, HIPMSELoss as MSELoss,
                           HIPSigmoid as Sigmoid, HIPLSTM as LSTM, HIPLayerNorm as LayerNorm, HIPGELU as GELU,
                           HIPCausalSelfAttention as CausalSelfAttention, KVCache, CrossAttentionMemory,
                           HIPConvTranspose2d as ConvTranspose2d, HIPBatchNorm1d as BatchNorm1d, HIPTanh as Tanh,
                           HIPBCELoss as BCELoss, HIPGRU as GRU, HIPRNN as RNN, HIPBidirectional as Bidirectional,
                           HIPSoftplus as Softplus, HIPSoftsign as Softsign, HIPMish as Mish, HIPTanhExp as TanhExp,
                           HIPELU as ELU, HIPSELU as SELU, HIPLogSoftmax as LogSoftmax, HIPNLLLoss as NLLLoss,
                           HIPL1Loss as L1Loss, HIPKLDivLoss as KLDivLoss, HIPAvgPool2d as AvgPool2d,
                           HIPZeroPad2d as ZeroPad2d, HIPFlatten as Flatten)


class CrossEntropyLoss(HIPCrossEntropyLoss):
    """neunet.nn.CrossEntropyLoss signature (losses.py:59-64): weight, ignore_index, reduction (default 'mean')."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean", inplace=False):
        super().__init__(reduction=reduction, ignore_index=ignore_index, inplace=inplace, weight=weight)
