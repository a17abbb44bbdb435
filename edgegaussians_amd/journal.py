"""The step journal of an EdgeTrainer: the enqueues since the last read-back, the trigger of the state snapshot in front of
them, and the call-tag counter of the chained forward.  A read-back that finds a sticky device flag raised restores the
snapshot and replays the entries (EdgeTrainer._recover_from_overflow).  Host only: device work goes through the trainer."""
from __future__ import annotations

from typing import List

from torch import Tensor

from ._lib import MAX_WS_TAG

# a window is read back before its replay could draw more tags than this (a replay reserves its tags up front)
WINDOW_TAGS = MAX_WS_TAG // 2


class Entry:
    """One journalled enqueue: `tags`, the fresh call tags its replay draws (at most); `steps`, what it counts towards the
    journal's length; `opens_window`, False for an entry journalled inside a window only.  `epoch` and `loss_scale` are
    stamped by the journal."""
    tags = steps = 1
    opens_window = True
    epoch, loss_scale, wmaps = 0, 1.0, ()


class Steps(Entry):
    """A run of single steps (train_step(s), a scene of train_steps_multi), replayed one step at a time."""

    def __init__(self, views, wmaps):
        self.views, self.wmaps, self.tags, self.steps = views, wmaps, len(views), len(views)

    def replay(self, tr) -> None:
        for v, w in zip(self.views, self.wmaps):
            tr._step_raw(v, w)


class Batched(Entry):
    """One optimizer step on the summed gradients of C views (train_step_batched)."""

    def __init__(self, views, wmaps):
        self.views, self.wmaps = views, wmaps

    def replay(self, tr) -> None:
        tr._batched_raw(self.views, self.wmaps, True)


class Regulariser(Entry):
    """A regulariser step with lambda from the device loss accumulator (no forward: no tags)."""
    tags = 0

    def __init__(self, kind: str, *settings):  # (scale_factor, dir_loss_num_nn, enforce_method)
        self.kind, self.settings = kind, settings

    def replay(self, tr) -> None:
        tr._regulariser_raw(self.kind, tr.loss_acc[0], *self.settings)


class EpochMark(Entry):
    """mark_epoch: the running loss sum parked in slot k."""
    tags, opens_window = 0, False

    def __init__(self, k: int):
        self.k = k

    def replay(self, tr) -> None:
        tr._mark_raw(self.k)


class DataParallel(Entry):
    """Data-parallel steps, replayed by every rank with their collectives.  A view is an int (one grad_step: one tag) or
    a list of views (two half batches: up to two tags)."""

    def __init__(self, views, wmaps, next_views):
        self.views, self.wmaps, self.next_views, self.steps = views, wmaps, next_views, len(views)
        self.tags = sum(1 if isinstance(v, int) else 2 for v in views)

    def replay(self, tr) -> None:
        for v, w, n in zip(self.views, self.wmaps, self.next_views):
            tr._dp._step_raw(v, w, n)


def chunks(views, *per_view, n: int = WINDOW_TAGS):
    """(views, *per_view) in slices of at most n steps: a run longer than a window is journalled and enqueued piecewise."""
    for i in range(0, len(views), n):
        yield (views[i:i + n],) + tuple(x[i:i + n] for x in per_view)


def _tensors(x):
    if isinstance(x, Tensor):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _tensors(y)


class StepJournal:
    """`tr` is the owning trainer: the journal calls its `_snapshot`, `_restore`, `flush`, `_zero_workspaces`, `_ctl_bits`
    and reads `epoch`, `loss_scale`."""

    def __init__(self, tr):
        self.tr, self.entries = tr, []  # type: List[Entry]
        self.tag = 0  # the last call tag handed out (eg_step_args.ws_tag: 1 .. MAX_WS_TAG)
        self._steps = self._tags = 0

    def __len__(self) -> int:
        return self._steps

    def bytes(self) -> int:
        """Bytes of the distinct weight maps the entries keep alive (the per-step `bg_edge_ratio` draws are fresh tensors:
        at 1600 x 1200 a window of 8 epochs holds ~0.7 GB of them); `train()` reads back early past 512 MB."""
        return sum({t.data_ptr(): t.numel() * t.element_size() for e in self.entries for t in _tensors(e.wmaps)}.values())

    def reserve(self, n: int) -> None:
        """Make sure n fresh, consecutive tags are left in 1 .. MAX_WS_TAG (16 bits: the forward's hand-over granules carry
        them) and that the window stays replayable: it is read back first if its entries and these n would draw more than
        WINDOW_TAGS.  When the range is used up (every 65 534 steps) the window is read back -- the sticky words of the
        control block are about to go --, the workspaces are zeroed and the tags start over, so that a granule written
        2^16 steps ago can never be mistaken for this call's."""
        assert 0 <= n <= WINDOW_TAGS, n
        tr = self.tr
        if self.entries and self._tags + n > WINDOW_TAGS:
            tr.flush()
        if self.tag + n > MAX_WS_TAG:
            if self.entries:
                tr.flush()
            elif tr._ctl_bits()[1]:  # nothing to replay, but the stall bit of control word 3 must not be zeroed unread
                raise RuntimeError(tr._STALL_MSG)
            tr._zero_workspaces()
            self.tag = 0

    def take(self, n: int) -> int:
        """First of n fresh, consecutive tags (reserved by the trainer's prologue; a bare grad_step reserves here)."""
        if self.tag + n > MAX_WS_TAG:
            self.reserve(n)
        self.tag += n
        return self.tag - n + 1

    def push(self, e: Entry) -> None:
        """Journal e; the first entry of a window snapshots the state in front of it."""
        if not self.entries:
            if not e.opens_window:
                return
            self.tr._snapshot()
        e.epoch, e.loss_scale = self.tr.epoch, self.tr.loss_scale
        self.entries.append(e)
        self._steps += e.steps
        self._tags += e.tags

    def clear(self) -> None:
        self.entries.clear()
        self._steps = self._tags = 0

    def replay(self) -> None:
        """Restore the snapshot and run the entries again, each with the epoch and loss scale it was journalled with, then
        put the current ones back.  The window's tags are reserved first: the range cannot wrap inside the replay."""
        tr = self.tr
        assert self._tags <= MAX_WS_TAG, "journal longer than the tag range"
        if self.tag + self._tags > MAX_WS_TAG:
            tr._zero_workspaces()
            self.tag = 0
        now = tr.epoch, tr.loss_scale
        tr._restore()  # (the running loss sum included)
        for e in list(self.entries):
            tr.epoch, tr.loss_scale = e.epoch, e.loss_scale
            e.replay(tr)
        tr.epoch, tr.loss_scale = now
