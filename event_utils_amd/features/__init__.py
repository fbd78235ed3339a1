from .corners import fast_corners, harris_scores, harris_corners, corner_events  # noqa: F401
from .plane_flow import local_plane_flow, plane_flow_field  # noqa: F401
