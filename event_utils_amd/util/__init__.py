from .event_util import events_bounds_mask, clip_events_to_bounds, get_events_from_mask, remove_hot_pixels  # noqa: F401
from .event_denoise import neighbour_support, background_activity_filter, refractory_filter  # noqa: F401
