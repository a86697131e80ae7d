"""Name-lookup namespace mirroring ``nntts.optimizers`` (reference nntts/bin/train.py:186-193).
`Adam`, `AdamW` and `RAdam` are the fused clip + update kernels of efficient_tts_amd.optim; they are constructed from the MODEL
(they re-home the parameters into one flat buffer), not from `model.parameters()`.  `RAdam` is the reference's own
(nntts/optimizers/radam.py), which that registry's star imports place over torch's."""
from .optim import EftsAdam as Adam  # noqa: F401
from .optim import EftsAdamW as AdamW  # noqa: F401
from .optim import EftsRAdam as RAdam  # noqa: F401
