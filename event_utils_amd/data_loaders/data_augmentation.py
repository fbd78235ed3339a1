"""Transforms of lib/data_loaders/data_augmentation.py: Compose, CenterCrop, RobustNorm.  RobustNorm runs on the GPU
(evk_robust_norm_f32: both percentiles by one radix select, clamp and min / max normalisation fused); a CPU tensor goes
there and comes back.  Each transform also applies to a whole batch of items at once (`batch`), which is what
BaseVoxelDataset.__getitems__ uses."""
import numbers

import torch

from . import _kernels as K

__all__ = ['Compose', 'CenterCrop', 'RobustNorm']


class Compose(object):
    """
    Composes several transforms together.
    """

    def __init__(self, transforms):
        """
        @param transforms (list of ``Transform`` objects): list of transforms to compose.
        """
        self.transforms = transforms

    def __call__(self, x, is_flow=False):
        for t in self.transforms:
            x = t(x, is_flow)
        return x

    def batch(self, x):
        """The transforms applied to every item x[k] of a batch tensor."""
        for t in self.transforms:
            x = t.batch(x)
        return x

    def __repr__(self):
        format_string = self.__class__.__name__ + '('
        for t in self.transforms:
            format_string += '\n'
            format_string += '    {0}'.format(t)
        format_string += '\n)'
        return format_string


class CenterCrop(object):
    """
    Center crop the tensor to a certain size.
    """

    def __init__(self, size, preserve_mosaicing_pattern=False):
        if isinstance(size, numbers.Number):
            self.size = (int(size), int(size))
        else:
            self.size = size

        self.preserve_mosaicing_pattern = preserve_mosaicing_pattern

    def offsets(self, h, w):
        """Top-left corner (i, j) of the crop of an h x w plane (data_augmentation.py:64-75)."""
        th, tw = self.size
        assert(th <= h)
        assert(tw <= w)
        i = int(round((h - th) / 2.))
        j = int(round((w - tw) / 2.))
        if self.preserve_mosaicing_pattern:
            # make sure that i and j are even, to preserve the mosaicing pattern
            if i % 2 == 1:
                i = i + 1
            if j % 2 == 1:
                j = j + 1
        return i, j

    def __call__(self, x, is_flow=False):
        """
            @param x [C x H x W] Tensor to be cropped.
            @param is_flow this parameter does not have any effect
            @returns Cropped tensor (a view).
        """
        i, j = self.offsets(x.shape[1], x.shape[2])
        th, tw = self.size
        return x[:, i:i + th, j:j + tw]

    def batch(self, x):
        i, j = self.offsets(x.shape[2], x.shape[3])
        th, tw = self.size
        return x[:, :, i:i + th, j:j + tw]

    def __repr__(self):
        return self.__class__.__name__ + '(size={0})'.format(self.size)


class RobustNorm(object):
    """
    Robustly normalize tensor (ie normalise it between top and
    bottom centiles of tensor value range)
    """

    def __init__(self, low_perc=0, top_perc=95):
        self.top_perc = top_perc
        self.low_perc = low_perc

    @staticmethod
    def percentile(t, q):
        """
        Return the ``q``-th percentile of the flattened input tensor's data: the value of rank 1 + round(.01 * q * (n - 1))
        in torch.kthvalue's order (not interpolated, numpy.percentile(..., interpolation="nearest")), found on the GPU.
        @param t Input tensor (float32).
        @param q Percentile to compute, which must be between 0 and 100 inclusive.
        @returns Resulting value (scalar).
        """
        return float(K.robust_norm(t, q, q)[1][0, 0].item())

    def __call__(self, x, is_flow=False):
        """
        Normalise x: (clamp(x, t_min, t_max) - min) / (max + 1e-6) with t_min, t_max its low / top percentiles; x itself
        when both are 0 (data_augmentation.py:131-146).
        """
        out, perc = K.robust_norm(x, self.low_perc, self.top_perc)
        lo, hi = perc[0].tolist()
        return x if (hi == 0 and lo == 0) else out

    def batch(self, x):
        """Every item x[k] normalised by one selection launch and one elementwise launch; an item whose percentiles are both 0 is
        copied unchanged."""
        return K.robust_norm(x, self.low_perc, self.top_perc, batch_dims=1)[0]

    def __repr__(self):
        format_string = self.__class__.__name__
        format_string += '(top_perc={:.2f}'.format(self.top_perc)
        format_string += ', low_perc={:.2f})'.format(self.low_perc)
        return format_string


# transform names of the dataset's `transforms` dict (base_dataset.py:190,195 evaluates them with eval)
TRANSFORMS = {'Compose': Compose, 'CenterCrop': CenterCrop, 'RobustNorm': RobustNorm}
