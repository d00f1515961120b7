"""HIP-accelerated layers: one-to-one counterparts of neunet/nn/experimental/*
(the reference's CUDA* classes are also exported as aliases of the HIP* ones)."""
from .activations import (CUDAFusedSwishAndMul, CUDASoftmax, CUDASwish, HIPFusedSwishAndMul, HIPGELU, HIPReLU,  # noqa: F401
                          HIPSoftmax, HIPSwish, HIPTanh, HIPSoftplus, HIPSoftsign, HIPMish, HIPTanhExp, HIPELU, HIPSELU,
                          HIPLogSoftmax)
from .linear import CUDALinear, HIPLinear  # noqa: F401
from .linear_swish import CUDALinearSwish, HIPLinearSwish  # noqa: F401
from .losses import CUDACrossEntropyLoss, HIPBCELoss, HIPCrossEntropyLoss, HIPKLDivLoss, HIPL1Loss, HIPNLLLoss  # noqa: F401
from .rmsnorm import CUDARMSNorm, HIPRMSNorm  # noqa: F401
from .conv2d import HIPConv2d  # noqa: F401
from .conv_transpose2d import HIPConvTranspose2d  # noqa: F401
from .attention import CrossAttentionMemory, HIPMultiHeadAttention  # noqa: F401
from .embedding import HIPDropout, HIPEmbedding, HIPPositionalEncoding  # noqa: F401
from .vision import HIPBatchNorm2d, HIPLeakyReLU, HIPMaxPool2d, HIPMSELoss, HIPSigmoid  # noqa: F401
from .recurrent import HIPLSTM, HIPGRU, HIPRNN, HIPBidirectional  # noqa: F401
from .layernorm import HIPLayerNorm  # noqa: F401
from .causal_attention import HIPCausalSelfAttention, KVCache  # noqa: F401
from .batchnorm1d import HIPBatchNorm1d  # noqa: F401
from .pooling import HIPAvgPool2d, HIPFlatten, HIPZeroPad2d  # noqa: F401
