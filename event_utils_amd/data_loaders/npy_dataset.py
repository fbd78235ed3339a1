"""NpyDataset of lib/data_loaders/npy_dataset.py: one (N, 4) array of [x, y, p, t (microseconds)] rows.
The columns are widened as the reference's loaders widen them (coordinates .astype(float32), p * 2 - 1, t * 1e-6 in
float64, each window's t - ts[0] in float64 before the float32 cast) and uploaded once.  Deviations, where the reference
cannot run: ts(index) reads the time stamps (upstream refers to an undefined name), and the inferred resolution is
(max y + 1, max x + 1) as MemMapDataset.infer_resolution gives it (upstream's [max x, max y] indexes out of range)."""
import numpy as np

from .base_dataset import BaseVoxelDataset

__all__ = ['NpyDataset']


class NpyDataset(BaseVoxelDataset):
    """
    Dataloader for events saved as a numpy (N, 4) array of x, y, p, t
    (see https://github.com/TimoStoff/event_utils for code to convert datasets)
    """

    def get_frame(self, index):
        return None

    def get_flow(self, index):
        return None

    def get_events(self, idx0, idx1):
        xs = self.xs[idx0:idx1]
        ys = self.ys[idx0:idx1]
        ts = self.ts[idx0:idx1]
        ps = self.ps[idx0:idx1]
        return xs, ys, ts, ps

    def resident_columns(self):
        return dict(xs=self.xs, ys=self.ys, ts=self.ts, ps=self.ps, p_pm1=False)

    def load_data(self, data_path):
        self.data = np.load(data_path)
        self.xs, self.ys, self.ps, self.ts = self.data[:, 0], self.data[:, 1], self.data[:, 2]*2-1, self.data[:, 3]*1e-6
        self._t_host = self.ts

        if self.sensor_resolution is None:
            self.sensor_resolution = [int(np.max(self.ys)) + 1, int(np.max(self.xs)) + 1]
        else:
            self.sensor_resolution = self.sensor_resolution[0:2]
        self.has_flow = False
        self.has_frames = False
        self.t0 = self.ts[0]
        self.tk = self.ts[-1]
        self.num_events = len(self.xs)
        self.num_frames = 0
        self.frame_ts = []

    def find_ts_index(self, timestamp):
        idx = np.searchsorted(self.ts, timestamp)
        return idx

    def ts(self, index):  # (shadowed by the time stamp array self.ts once load_data has run, as upstream)
        return self._t_host[index]

    def compute_frame_indices(self):
        return None
