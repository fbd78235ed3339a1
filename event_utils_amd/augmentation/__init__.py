from .event_augmentation import (sample, events_to_block, merge_events, add_random_events, remove_events,  # noqa: F401
                                 add_correlated_events, flip_events_x, flip_events_y, crop_events, rotate_events)
