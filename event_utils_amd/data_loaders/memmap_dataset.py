"""MemMapDataset of lib/data_loaders/memmap_dataset.py: the RPG memmap format (a directory of t.npy, xy.npy, p.npy and
optionally images.npy, timestamps.npy, optic_flow.npy, optic_flow_stamps.npy, dataset_config.json).  The event columns
go to the GPU once, in their stored dtypes; the memory maps stay open for the window tables, time stamps and frames.
Deviations, where the reference cannot run: find_config reads dataset_config.json itself (upstream calls read_json
without importing it), and a directory without images.npy is accepted (has_frames=False, no frames)."""
import json
import os

import numpy as np

from .base_dataset import BaseVoxelDataset

__all__ = ['MemMapDataset']


class MemMapDataset(BaseVoxelDataset):
    """
    Dataloader for events saved in the MemMap events format used at RPG.
    (see https://github.com/TimoStoff/event_utils for code to convert datasets)
    """

    def get_frame(self, index):
        frame = self.filehandle['images'][index][:, :, 0]
        return frame

    def get_flow(self, index):
        flow = self.filehandle['optic_flow'][index]
        return flow

    def get_events(self, idx0, idx1):
        xy = self.filehandle["xy"][idx0:idx1]
        xs = xy[:, 0].astype(np.float32)
        ys = xy[:, 1].astype(np.float32)
        ts = self.filehandle["t"][idx0:idx1]
        ps = self.filehandle["p"][idx0:idx1] * 2.0 - 1.0
        return xs, ys, ts, ps

    def resident_columns(self):
        return dict(xy=self.filehandle["xy"], ts=self.filehandle["t"], ps=self.filehandle["p"], p_pm1=True)

    def load_data(self, data_path, timestamp_fname="timestamps.npy", image_fname="images.npy",
                  optic_flow_fname="optic_flow.npy", optic_flow_stamps_fname="optic_flow_stamps.npy",
                  t_fname="t.npy", xy_fname="xy.npy", p_fname="p.npy"):

        assert os.path.isdir(data_path), '%s is not a valid data_path' % data_path

        data = {}
        self.has_flow = False
        for subroot, _, fnames in sorted(os.walk(data_path)):
            for fname in sorted(fnames):
                path = os.path.join(subroot, fname)
                if fname.endswith(".npy"):
                    if fname.endswith(timestamp_fname):
                        frame_stamps = np.load(path)
                        data["frame_stamps"] = frame_stamps
                    elif fname.endswith(image_fname):
                        data["images"] = np.load(path, mmap_mode="r")
                    elif fname.endswith(optic_flow_fname):
                        data["optic_flow"] = np.load(path, mmap_mode="r")
                        self.has_flow = True
                    elif fname.endswith(optic_flow_stamps_fname):
                        optic_flow_stamps = np.load(path)
                        data["optic_flow_stamps"] = optic_flow_stamps

                    handle = np.load(path, mmap_mode="r")
                    if fname.endswith(t_fname):  # timestamps
                        data["t"] = handle.squeeze()
                    elif fname.endswith(xy_fname):  # coordinates
                        data["xy"] = handle.squeeze()
                    elif fname.endswith(p_fname):  # polarity
                        data["p"] = handle.squeeze()
            if len(data) > 0:
                data['path'] = subroot
                if "t" not in data:
                    continue
                assert (len(data['p']) == len(data['xy']) and len(data['p']) == len(data['t']))

                self.t0, self.tk = data['t'][0], data['t'][-1]
                self.num_events = len(data['p'])
                if "images" not in data:                 # (deviation: upstream needs images.npy)
                    self.has_frames = False
                self.num_frames = len(data['images']) if "images" in data else 0

                self.frame_ts = []
                for ts in data.get("frame_stamps", []):
                    self.frame_ts.append(ts)
                data["index"] = self.frame_ts

        self.filehandle = data
        self._t_host = data["t"] if "t" in data else None
        self.find_config(data_path)

    def find_ts_index(self, timestamp):
        index = np.searchsorted(self.filehandle["t"], timestamp)
        return index

    def ts(self, index):
        return self.filehandle["t"][index]

    def infer_resolution(self):
        if len(self.filehandle.get("images", [])) > 0:
            sr = self.filehandle["images"][0].shape[0:2]
        else:
            sr = [np.max(self.filehandle["xy"][:, 1]) + 1, np.max(self.filehandle["xy"][:, 0]) + 1]
        return sr

    def find_config(self, data_path):
        if self.sensor_resolution is None:
            config = os.path.join(data_path, "dataset_config.json")
            if os.path.exists(config):
                with open(config) as f:
                    self.config = json.load(f)
                self.data_source = self.config['data_source']
                self.sensor_resolution = self.config["sensor_resolution"]
            else:
                data_source = 'unknown'  # noqa: F841 (upstream)
                self.sensor_resolution = self.infer_resolution()
