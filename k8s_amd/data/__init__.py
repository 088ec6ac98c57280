"""Training on a dataset: the on-disk format (``dataset``), the sampler and augmentation tables (``sampler``) and
the loader that ends in the fused augmentation kernel (``loader``)."""
from k8s_amd.data.dataset import DataError, Dataset, open_dataset, write_dataset  # noqa: F401
