"""Aliases under the reference's dotted paths: event_utils_amd.lib.representations.image, ...contrast_max.warps, ..."""
import sys as _sys

from .. import augmentation, calibration, contrast_max, data_formats, data_loaders, depth, features, representations, simulation, transforms, util, visualization  # noqa: F401

for _name, _mod in (("representations", representations), ("contrast_max", contrast_max), ("util", util),
                    ("transforms", transforms), ("visualization", visualization), ("augmentation", augmentation),
                    ("data_loaders", data_loaders), ("features", features), ("simulation", simulation), ("depth", depth),
                    ("calibration", calibration), ("data_formats", data_formats)):
    _sys.modules[__name__ + "." + _name] = _mod
    for _sub in ("image", "voxel_grid", "time_surface", "reconstruction", "event_simulator", "emvs", "stereo", "sgm", "tracking", "fusion", "camera", "raw", "corners", "plane_flow", "warps", "objectives", "events_cmax", "segmentation", "event_util", "event_denoise", "optic_flow", "draw_flow",
                 "event_augmentation", "base_dataset", "memmap_dataset", "npy_dataset", "data_augmentation", "dataloader_util"):
        if hasattr(_mod, _sub):
            _sys.modules[__name__ + "." + _name + "." + _sub] = getattr(_mod, _sub)
