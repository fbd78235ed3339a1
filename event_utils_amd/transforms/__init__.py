from .optic_flow import warp_events_flow_torch  # noqa: F401
from .flow_loss import flow_field_timestamp_images, flow_field_timestamp_loss, flow_timestamp_loss  # noqa: F401
from .flow_loss import flow_contrast_loss, flow_field_contrast_loss, flow_field_iwe  # noqa: F401
