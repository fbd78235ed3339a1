"""
event_utils_amd -- MI355X-native (gfx950 / CDNA4) implementation of the data-parallel core of TimoStoff/event_utils:
event -> image / voxel-grid binning (lib/representations) and linear-flow contrast maximisation (lib/contrast_max).
Python keeps the reference's function signatures; all event arithmetic runs in hand-written HIP kernels behind the
C ABI of include/evk.h (libevk.so).  There is no CPU fallback.

Module map (reference module -> here):
    lib.representations.image       -> event_utils_amd.representations.image
    lib.representations.voxel_grid  -> event_utils_amd.representations.voxel_grid
    (no reference module)           -> event_utils_amd.representations.time_surface (time_surfaces, local_time_surfaces,
                                                                             averaged_time_surfaces)
    (no reference module)           -> event_utils_amd.representations.reconstruction (leaky_integrator, complementary_filter,
                                                                             log_intensity, to_intensity)
    (no reference module)           -> event_utils_amd.simulation.event_simulator (simulate_events, SimulatorState)
    (no reference module)           -> event_utils_amd.depth.emvs           (dsi_votes, dsi_depth_map, emvs_depth_map,
                                                                             packet_transforms, depth_planes, depth_to_points)
    (no reference module)           -> event_utils_amd.depth.stereo         (quantised_time_surfaces, stereo_cost_volume,
                                                                             stereo_match, stereo_disparity, disparity_to_depth,
                                                                             disparity_depth_map)
    (no reference module)           -> event_utils_amd.depth.sgm            (sgm_aggregate, match_cost_volume, sgm_match,
                                                                             sgm_disparity)
    (no reference module)           -> event_utils_amd.depth.tracking       (tracking_surface, reference_points,
                                                                             registration_terms, registration_residuals,
                                                                             register_points, track_poses)
    (no reference module)           -> event_utils_amd.depth.fusion         (disparity_inverse_depth, depth_inverse_depth,
                                                                             inverse_depth_depth_map, relative_transforms,
                                                                             propagate_inverse_depth, fuse_inverse_depth,
                                                                             regularise_inverse_depth, fuse_stereo_depth)
    (no reference module)           -> event_utils_amd.calibration.camera   (CameraModel, RectificationMaps, distort_points,
                                                                             undistort_points, rectification_maps, rectify_events,
                                                                             remap_images, stereo_rectify)
    (lib.data_formats: HDF5, rosbag)-> event_utils_amd.data_formats.raw     (read_raw, write_raw, decode_evt3, decode_evt2,
                                                                             decode_raw, iter_decode_raw, encode_evt3, encode_evt2)
    lib.contrast_max.warps          -> event_utils_amd.contrast_max.warps
    lib.contrast_max.objectives     -> event_utils_amd.contrast_max.objectives
    lib.contrast_max.events_cmax    -> event_utils_amd.contrast_max.events_cmax
    lib.util.event_util             -> event_utils_amd.util.event_util      (events_bounds_mask, clip_events_to_bounds,
                                                                             get_events_from_mask, remove_hot_pixels)
    (no reference module)           -> event_utils_amd.util.event_denoise   (neighbour_support, background_activity_filter,
                                                                             refractory_filter)
    (no reference module)           -> event_utils_amd.features.corners     (fast_corners, harris_scores, harris_corners,
                                                                             corner_events)
    (no reference module)           -> event_utils_amd.features.plane_flow  (local_plane_flow, plane_flow_field)
    lib.augmentation.event_augmentation -> event_utils_amd.augmentation.event_augmentation (add_random_events,
                                                                             remove_events, add_correlated_events, ...)
(`event_utils_amd.lib.*` aliases the same modules under the reference's own dotted paths.)
"""
from .representations import *  # noqa: F401,F403
from .contrast_max.warps import warp_function, linvel_warp, warp_events, pure_rotation_warp, xyztheta_warp, \
    angular_velocity_warp, planar_flow_warp  # noqa: F401
from .contrast_max.objectives import objective_function, variance_objective, get_iwe, zhu_timestamp_objective, \
    get_timestamp_images  # noqa: F401
from .contrast_max.events_cmax import optimize, optimize_contrast  # noqa: F401
from .contrast_max.segmentation import cluster_iwes, segmentation_loss, update_assignments, segment_events, \
    SegmentationResult  # noqa: F401
from .util.event_util import events_bounds_mask, clip_events_to_bounds, get_events_from_mask, remove_hot_pixels  # noqa: F401
from .util.event_denoise import neighbour_support, background_activity_filter, refractory_filter  # noqa: F401
from .features.corners import fast_corners, harris_scores, harris_corners, corner_events  # noqa: F401
from .features.plane_flow import local_plane_flow, plane_flow_field  # noqa: F401
from .augmentation.event_augmentation import add_random_events, remove_events, add_correlated_events  # noqa: F401
from .simulation import simulate_events, SimulatorState  # noqa: F401
from .depth import DSI, DepthMap, depth_planes, packet_transforms, packet_times, dsi_votes, dsi_depth_map, emvs_depth_map, \
    depth_to_points  # noqa: F401
from .depth import Disparity, quantised_time_surfaces, stereo_cost_volume, stereo_match, stereo_disparity, disparity_to_depth, \
    disparity_depth_map  # noqa: F401
from .depth import sgm_aggregate, match_cost_volume, sgm_match, sgm_disparity  # noqa: F401
from .depth import Registration, tracking_surface, reference_points, registration_terms, registration_residuals, register_points, \
    track_poses  # noqa: F401
from .depth import InverseDepthMap, disparity_inverse_depth, depth_inverse_depth, inverse_depth_depth_map, relative_transforms, \
    propagate_inverse_depth, fuse_inverse_depth, regularise_inverse_depth, fuse_stereo_depth  # noqa: F401
from .calibration import CameraModel, RectificationMaps, distort_points, undistort_points, rectification_maps, rectify_events, \
    remap_images, stereo_rectify  # noqa: F401
from .data_formats import RawFile, RawEvents, RawStats, RawState, read_raw, write_raw, decode_evt3, decode_evt2, decode_raw, \
    iter_decode_raw, encode_evt3, encode_evt2  # noqa: F401
from .transforms import flow_field_timestamp_images, flow_field_timestamp_loss, flow_timestamp_loss  # noqa: F401
from .transforms import flow_contrast_loss, flow_field_contrast_loss, flow_field_iwe  # noqa: F401
from .events import DeviceEvents  # noqa: F401
from ._device import check_errors, error_mode  # noqa: F401
from .tiled import release_scratch  # noqa: F401

__version__ = "0.1.0"
