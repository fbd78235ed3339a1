from . import camera  # noqa: F401
from .camera import CameraModel, RectificationMaps, distort_points, undistort_points, rectification_maps, rectify_events, \
    remap_images, stereo_rectify  # noqa: F401
