"""lib/data_loaders on the GPU: event-window datasets whose voxel grids and RobustNorm run in libevk.so.
DynamicH5Dataset (hdf5_dataset.py) is not provided: h5py is not a dependency of this package."""
from . import base_dataset, data_augmentation, dataloader_util, memmap_dataset, npy_dataset  # noqa: F401
from .base_dataset import BaseVoxelDataset
from .data_augmentation import CenterCrop, Compose, RobustNorm
from .dataloader_util import unpack_batched_events
from .memmap_dataset import MemMapDataset
from .npy_dataset import NpyDataset

__all__ = ["BaseVoxelDataset", "MemMapDataset", "NpyDataset", "Compose", "CenterCrop", "RobustNorm", "unpack_batched_events"]
