"""BaseVoxelDataset of lib/data_loaders/base_dataset.py with the event stream resident on the GPU.

The stream is uploaded once, at construction; the host keeps its columns for the window tables, the time stamps and the
frames.  An item's voxel grid comes from evk_voxel_windows_f32 (one launch for one item, or for the whole batch in
__getitems__, which torch.utils.data.DataLoader calls when num_workers=0), RobustNorm from evk_robust_norm_f32.  Voxel grids
and events stay on the GPU; frames and flow are read and transformed on the host as upstream.  Reference quirks kept
(data loaders): between_frames clips the end index to num_events - 1, t_seconds / fixed_frames windows start at
the previous window's end, k_events windows overlap and an out-of-range window raises Exception, the length cap is
max_length + 1, an empty window is one zero event (NaN cells)."""
import random

import numpy as np
import torch
from torch.utils.data import Dataset
from torch.utils.data.dataloader import default_collate

from . import _kernels as K
from .data_augmentation import TRANSFORMS, Compose, CenterCrop, RobustNorm  # noqa: F401

__all__ = ['BaseVoxelDataset']

data_sources = ('esim', 'ijrr', 'mvsec', 'eccd', 'hqfd', 'unknown')


def _make_transform(name, kwargs):
    if name not in TRANSFORMS:
        raise ValueError("unknown transform %r (known: %s)" % (name, ", ".join(sorted(TRANSFORMS))))
    return TRANSFORMS[name](**kwargs)


class BaseVoxelDataset(Dataset):
    """
    Dataloader for voxel grids given file containing events.
    Also loads time-synchronized frames and optic flow if available.
    Voxel grids are formed on-the-fly, on the GPU.
    Subclasses implement get_frame, get_flow, get_events, load_data, find_ts_index, ts (as upstream) and
    resident_columns() -> dict(xy= or xs=/ys=, ts=, ps=, p_pm1=) of the stream as stored.
    Parameters: see the reference (base_dataset.py:117-153); voxel_method e.g.
        {'method':'k_events', 'k':10000, 'sliding_window_w':100}, {'method':'t_seconds', 't':0.5, 'sliding_window_t':0.1},
        {'method':'between_frames'}, {'method':'fixed_frames', 'num_frames':100}.
    """

    def get_frame(self, index):
        raise NotImplementedError

    def get_flow(self, index):
        raise NotImplementedError

    def get_events(self, idx0, idx1):
        raise NotImplementedError

    def load_data(self, data_path):
        raise NotImplementedError

    def find_ts_index(self, timestamp):
        raise NotImplementedError

    def ts(self, index):
        raise NotImplementedError

    def resident_columns(self):
        """The stream as stored, for its upload: dict(xy=(N, 2) or xs=, ys=, ts=, ps=, p_pm1=True when ps holds {0, 1}
        and the loader's get_events returns 2p - 1).  load_data also sets self._t_host, the host time stamps."""
        raise NotImplementedError

    def __init__(self, data_path, transforms={}, sensor_resolution=None, num_bins=5,
                 voxel_method={'method': 'between_frames'}, max_length=None, combined_voxel_channels=False,
                 return_events=False, return_voxelgrid=True, return_frame=True, return_prev_frame=False,
                 return_flow=True, return_prev_flow=False, return_format='torch'):
        self.num_bins = num_bins
        self.data_path = data_path
        self.combined_voxel_channels = combined_voxel_channels
        self.sensor_resolution = sensor_resolution
        self.data_source_idx = -1
        self.has_flow = False
        self.has_frames = True
        self.return_format = return_format
        self.counter = 0

        self.return_events = return_events
        self.return_voxelgrid = return_voxelgrid
        self.return_frame = return_frame
        self.return_prev_frame = return_prev_frame
        self.return_flow = return_flow
        self.return_prev_flow = return_prev_flow

        self.sensor_resolution, self.t0, self.tk, self.num_events, self.frame_ts, self.num_frames = \
            None, None, None, None, None, None

        self.load_data(data_path)

        if self.sensor_resolution is None or self.has_flow is None or self.t0 is None \
                or self.tk is None or self.num_events is None or self.frame_ts is None \
                or self.num_frames is None:
            raise Exception("Dataloader failed to intialize all required members")

        self.num_pixels = self.sensor_resolution[0] * self.sensor_resolution[1]
        self.duration = self.tk - self.t0

        self.set_voxel_method(voxel_method)

        # transforms (base_dataset.py:188-204): with RobustNorm, the voxels get every transform and the frames / flow every
        # transform but RobustNorm.  The caller's dict is not modified.
        transforms = dict(transforms)
        self.normalize_voxels = False
        if 'RobustNorm' in transforms.keys():
            vox_transforms_list = [_make_transform(t, kwargs) for t, kwargs in transforms.items()]
            del (transforms['RobustNorm'])
            self.normalize_voxels = True
            self.vox_transform = Compose(vox_transforms_list)

        transforms_list = [_make_transform(t, kwargs) for t, kwargs in transforms.items()]

        if len(transforms_list) == 0:
            self.transform = None
        elif len(transforms_list) == 1:
            self.transform = transforms_list[0]
        else:
            self.transform = Compose(transforms_list)
        if not self.normalize_voxels:
            self.vox_transform = self.transform

        if max_length is not None:
            self.length = min(self.length, max_length + 1)

        self.stream = K.ResidentStream(**self.resident_columns()) if self.return_voxelgrid or self.return_events else None

    @staticmethod
    def preprocess_events(xs, ys, ts, ps):
        """
        Given empty events, return single zero event
        """
        if len(xs) == 0:
            txs = np.zeros((1))
            tys = np.zeros((1))
            tts = np.zeros((1))
            tps = np.zeros((1))
            return txs, tys, tts, tps
        return xs, ys, ts, ps

    def _window_times(self, idx0, idx1):
        """ts[0], ts[-1] of the window as get_events + preprocess_events return them (0.0 for an empty window)."""
        if idx1 <= idx0:
            return np.float64(0.0), np.float64(0.0)
        return self._t_host[idx0], self._t_host[idx1 - 1]

    def __getitem__(self, index, seed=None):
        """
        Get data at index.
        @param index Index of data
        @param seed Random seed for data augmentation
        @returns Dict with desired outputs (voxel grid, events, frames etc) as set in constructor
        """
        return self._items([index], [seed], batched=False)[0]

    def __getitems__(self, indices):
        """A whole batch: every voxel grid of it from one launch, RobustNorm over the batch in one launch.  Returns the per-item
        dicts; their voxel / event tensors are views of the batch allocation."""
        return self._items(list(indices), [None] * len(indices), batched=True)

    def _items(self, indices, seeds, batched):
        for index in indices:
            if index < 0 or index >= self.__len__():
                raise IndexError
        seeds = [random.randint(0, 2 ** 32) if s is None else s for s in seeds]
        windows = [self.get_event_indices(index) for index in indices]
        items = []
        for index, (idx0, idx1) in zip(indices, windows):
            ts_0, ts_k = self._window_times(idx0, idx1)
            dt = ts_k - ts_0
            items.append({'data_source_idx': self.data_source_idx, 'data_path': self.data_path,
                          'timestamp': ts_k, 'dt_between_frames': dt, 'ts_idx0': ts_0, 'ts_idx1': ts_k,
                          'idx0': idx0, 'idx1': idx1})
        if self.return_voxelgrid:
            vox = self.stream.voxel_windows(windows, self.num_bins, self.sensor_resolution,
                                            split=not self.combined_voxel_channels)
            if batched:
                if self.vox_transform:
                    random.seed(seeds[-1])
                    vox = self.vox_transform.batch(vox)
                for k, item in enumerate(items):
                    item['voxel'] = vox[k]
            else:
                items[0]['voxel'] = self.transform_voxel(vox[0], seeds[0])

        for k, index in enumerate(indices):
            self._frames_and_flow(items[k], index, seeds[k])

        if self.return_events:
            self._events(items, windows)
        return items

    def _frames_and_flow(self, item, index, seed):
        dt = item['dt_between_frames']
        if self.voxel_method['method'] == 'between_frames':
            frame = self.get_frame(index)
            frame = self.transform_frame(frame, seed)

            if self.has_flow:
                flow = self.get_flow(index)
                # convert to displacement (pix)
                flow = flow * dt
                flow = self.transform_flow(flow, seed)
            else:
                if self.return_format == 'torch':
                    flow = torch.zeros((2, frame.shape[-2], frame.shape[-1]), dtype=frame.dtype, device=frame.device)
                else:
                    flow = np.zeros((2, frame.shape[-2], frame.shape[-1]))

            if self.return_flow:
                item['flow'] = flow
                item['flow_ts'] = self.frame_ts[index]
            if self.return_prev_flow:
                prev_flow = flow if not self.has_flow else self.get_flow(index)
                item['prev_flow'] = self.transform_flow(prev_flow, seed)
            if self.return_frame:
                item['frame'] = frame
                item['frame_ts'] = self.frame_ts[index]
            if self.return_prev_frame:
                item['prev_frame'] = self.transform_frame(self.get_frame(index), seed)
        else:
            frames = []
            frame_ts = []
            if self.has_frames and self.return_frame:
                fi = self.frame_indices[index]
                if fi[0] != -1:
                    # (upstream reads frames 0 .. fi[1]-fi[0]-1, not fi[0] .. fi[1]-1: kept, base_dataset.py:284)
                    frames = [self.transform_frame(self.get_frame(fidx), seed) for fidx in range(fi[1]-fi[0])]
                    frame_ts = self.frame_ts[fi[0]:fi[1]]
            item['frame'] = frames
            item['frame_ts'] = frame_ts

            flows = []
            flow_ts = []
            if self.has_flow and self.return_flow:
                fi = self.frame_indices[index]
                if fi[0] != -1 and self.has_flow:
                    flows = [self.transform_flow(self.get_flow(fidx), seed) for fidx in range(fi[0], fi[1], 1)]
                    flow_ts = self.frame_ts[fi[0]:fi[1]]
            item['flow'] = flows
            item['flow_ts'] = flow_ts

    def _events(self, items, windows):
        if self.return_format == 'torch':
            packed, rows, lens = self.stream.pack_events(windows)
            for item, (idx0, idx1), r, n in zip(items, windows, rows.tolist(), lens.tolist()):
                if idx0-idx1 == 0:
                    item['events'] = torch.zeros((1, 4), dtype=torch.float32, device=self.stream.device)
                    item['events_batch_indices'] = torch.ones((1))
                    item['ts_idx0'] = torch.zeros((1), dtype=torch.float64)
                else:
                    item['events'] = packed[r:r + n]
                    item['events_batch_indices'] = idx1-idx0
                    item['ts_idx0'] = torch.tensor(item['ts_idx0'])
        elif self.return_format == 'numpy':
            for item, (idx0, idx1) in zip(items, windows):
                if idx0-idx1 == 0:
                    item['events'] = np.zeros((1, 4))
                    item['events_batch_indices'] = np.ones((1))
                    item['ts_idx0'] = np.zeros((1))
                else:
                    xs, ys, ts, ps = self.get_events(idx0, idx1)
                    item['events'] = np.stack((xs, ys, ts, ps), axis=1)
                    item['events_batch_indices'] = idx1-idx0
                    item['ts_idx0'] = np.array(item['ts_idx0'])
        else:
            raise Exception("Invalid event format '{}' used".format(self.return_format))

    def compute_between_frame_indices(self):
        """
        For each frame, find the start and end indices of the time synchronized events
        """
        frame_indices = []
        start_idx = 0
        for ts in self.frame_ts:
            end_index = self.find_ts_index(ts)
            if end_index >= self.num_events:
                end_index = self.num_events-1
            frame_indices.append([start_idx, end_index])
            start_idx = end_index
        return frame_indices

    def compute_timeblock_indices(self):
        """
        For each block of time (using t_seconds), find the start and end indices of the corresponding events
        """
        timeblock_indices = []
        start_idx = 0
        for i in range(self.__len__()):
            start_time = ((self.voxel_method['t'] - self.voxel_method['sliding_window_t']) * i) + self.t0
            end_time = start_time + self.voxel_method['t']
            end_idx = self.find_ts_index(end_time)
            timeblock_indices.append([start_idx, end_idx])
            start_idx = end_idx
        return timeblock_indices

    def compute_k_indices(self):
        """
        For each block of k events, find the start and end indices of the corresponding events (with sliding window)
        """
        k_indices = []
        for i in range(self.__len__()):
            idx0 = (self.voxel_method['k'] - self.voxel_method['sliding_window_w']) * i
            idx1 = idx0 + self.voxel_method['k']
            k_indices.append([idx0, idx1])
        return k_indices

    def compute_per_frame_indices(self):
        """
        For each set of event_indices, find the enclosed frame indices
        """
        frame_indices = []
        for indices in self.event_indices:
            s_t, e_t = self.ts(int(indices[0])), self.ts(int(indices[1]))
            idx0 = min(np.searchsorted(self.frame_ts, s_t), len(self.frame_ts)-1)
            idx1 = min(np.searchsorted(self.frame_ts, e_t), len(self.frame_ts)-1)
            if idx0 == idx1:
                frame_indices.append([-1, -1])
            else:
                frame_indices.append([idx0, idx1])
        return frame_indices

    def set_voxel_method(self, voxel_method):
        """
        Given the desired method of computing voxels, compute the event_indices lookup table and dataset length
        """
        self.voxel_method = voxel_method
        if self.voxel_method['method'] == 'k_events':
            self.length = max(int(self.num_events / (voxel_method['k'] - voxel_method['sliding_window_w'])), 0)
            self.event_indices = self.compute_k_indices()
        elif self.voxel_method['method'] == 't_seconds':
            self.length = max(int(self.duration / (voxel_method['t'] - voxel_method['sliding_window_t'])), 0)
            self.event_indices = self.compute_timeblock_indices()
        elif self.voxel_method['method'] == 'fixed_frames':
            self.length = self.voxel_method['num_frames']
            self.voxel_method['t'] = (self.tk-self.t0)/self.length
            voxel_method['sliding_window_t'] = 0
            self.event_indices = self.compute_timeblock_indices()
        elif self.voxel_method['method'] == 'between_frames':
            self.length = self.num_frames - 1
            self.event_indices = self.compute_between_frame_indices()
        else:
            raise Exception("Invalid voxel forming method chosen ({})".format(self.voxel_method))
        if self.has_frames:
            self.frame_indices = self.compute_per_frame_indices()
        if self.length == 0:
            raise Exception("Current voxel generation parameters lead to sequence length of zero")

    def __len__(self):
        return self.length

    def get_event_indices(self, index):
        """
        Get start and end indices of events at index
        """
        idx0, idx1 = self.event_indices[index]
        if not (idx0 >= 0 and idx1 <= self.num_events):
            raise Exception("WARNING: Event indices {},{} out of bounds 0,{}".format(idx0, idx1, self.num_events))
        return int(idx0), int(idx1)

    def get_voxel_grid(self, xs, ys, ts, ps, combined_voxel_channels=True):
        """
        Given events (torch tensors or numpy arrays, already widened to float32 with t relative to the window), return the
        voxel grid: NUM_BINS x H x W (combined) or 2*NUM_BINS x H x W (positive, then negative events), on the GPU.
        """
        from ..representations.voxel_grid import events_to_neg_pos_voxel_torch, events_to_voxel_torch
        cols = [c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))
                for c in (xs, ys, ts, ps)]
        cols = [c.cuda() for c in cols]
        if combined_voxel_channels:
            return events_to_voxel_torch(*cols, self.num_bins, sensor_size=self.sensor_resolution)
        voxel_grid = events_to_neg_pos_voxel_torch(*cols, self.num_bins, sensor_size=self.sensor_resolution)
        return torch.cat([voxel_grid[0], voxel_grid[1]], 0)

    def transform_frame(self, frame, seed):
        """
        Augment frame and turn into tensor
        """
        if self.return_format == "torch":
            frame = torch.from_numpy(frame).float().unsqueeze(0) / 255
            if self.transform:
                random.seed(seed)
                frame = self.transform(frame)
        return frame

    def transform_voxel(self, voxel, seed):
        """
        Augment voxel
        """
        if self.vox_transform:
            random.seed(seed)
            voxel = self.vox_transform(voxel)
        return voxel

    def transform_flow(self, flow, seed):
        """
        Augment flow and turn into tensor
        """
        if self.return_format == "torch":
            flow = torch.from_numpy(flow)  # should end up [2 x H x W]
            if self.transform:
                random.seed(seed)
                flow = self.transform(flow, is_flow=True)
        return flow

    def size(self):
        """
        Get the size of the event camera sensor/resolution
        """
        return self.sensor_resolution

    @staticmethod
    def unpackage_events(events):
        """
        Given events as 2D array, break it up into xs,ys,ts,ps components
        """
        return events[:,0], events[:,1], events[:,2], events[:,3]

    @staticmethod
    def collate_fn(data, event_keys=['events'], idx_keys=['events_batch_indices']):
        """
        Custom collate function for pyTorch batching to allow batching events
        """
        collated_events = {}
        events_arr = []
        end_idx = 0
        batch_end_indices = []
        for idx, item in enumerate(data):
            for k, v in item.items():
                if not k in collated_events.keys():
                    collated_events[k] = []
                if k in event_keys:
                    end_idx += v.shape[0]
                    events_arr.append(v)
                    batch_end_indices.append(end_idx)
                else:
                    collated_events[k].append(v)
        for k in collated_events.keys():
            try:
                i = event_keys.index(k)
                events = torch.cat(events_arr, dim=0)
                collated_events[event_keys[i]] = events
                collated_events[idx_keys[i]] = batch_end_indices
            except:
                collated_events[k] = default_collate(collated_events[k])
        return collated_events
