from . import event_simulator  # noqa: F401
from .event_simulator import simulate_events, SimulatorState  # noqa: F401
