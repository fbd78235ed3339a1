"""lib/data_loaders/dataloader_util.py."""
import torch

__all__ = ['unpack_batched_events']


def unpack_batched_events(events, batch_indices):
    """
    When returning events from a pytorch dataloader, it is often convenient when batching, to place them into a contiguous
    Nx4 array (collate_fn), where N = the length of all B event arrays in the batch.  This function unpacks the events into a
    Bx1xMx4 array, where M is the length of the *longest* event array in the batch; the shorter ones are padded with zeros.
    (Upstream's body refers to undefined names; this is what its docstring states.)
    @param events (N, 4) (or 1x1xNx4) array of the events
    @param batch_indices the end index of each event array: for two arrays of 200 and 700 events, [200, 900]
    @returns unpacked_events: Bx1xMx4 tensor, on the device of `events`
    """
    events = events.reshape(-1, 4)
    ends = [int(e) for e in batch_indices]
    starts = [0] + ends[:-1]
    maxlen = max([e - s for s, e in zip(starts, ends)] + [0])
    unpacked_events = torch.zeros((len(ends), 1, maxlen, 4), dtype=events.dtype, device=events.device)
    for b_idx, (s, e) in enumerate(zip(starts, ends)):
        unpacked_events[b_idx, 0, 0:e - s, :] = events[s:e, :]
    return unpacked_events
