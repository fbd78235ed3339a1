"""Recording formats (the reference's lib/data_formats is HDF5 and rosbag only): Prophesee EVT3 / EVT2 .raw files, decoded on the
device."""
from . import raw  # noqa: F401
from .raw import RawFile, RawEvents, RawStats, RawState, read_raw, write_raw, parse_raw_header, decode_evt3, decode_evt2, \
    decode_raw, iter_decode_raw, encode_evt3, encode_evt2  # noqa: F401
