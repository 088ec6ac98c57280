"""Training on a dataset: the on-disk format (``dataset``), the sampler and augmentation tables (``sampler``) and
the loader that ends in the fused augmentation kernel (``loader``); for token models the token format (``tokens``),
its sampler (``token_sampler``) and the loader that ends in the fused MLM / causal batch kernels (``token_loader``)."""
from k8s_amd.data.dataset import DataError, Dataset, open_dataset, write_dataset  # noqa: F401
from k8s_amd.data.tokens import TokenDataset, dataset_kind, open_token_dataset, write_token_dataset  # noqa: F401
