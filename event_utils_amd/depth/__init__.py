from . import emvs  # noqa: F401
from .emvs import DSI, DepthMap, depth_planes, packet_transforms, packet_times, dsi_votes, dsi_depth_map, emvs_depth_map, \
    depth_to_points  # noqa: F401
