from .corners import fast_corners, harris_scores, harris_corners, corner_events  # noqa: F401
