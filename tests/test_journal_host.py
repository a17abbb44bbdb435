"""The step journal (edgegaussians_amd/journal.py) behind EdgeTrainer's enqueue prologue, on the host: the tag cost of each
entry kind, the chunking of long runs, the tag wrap, the snapshot trigger, epoch marks and the order of a replay.  The
trainer's own prologue and entry points run; the device work is replaced by recording stand-ins.  No GPU."""
import torch

from edgegaussians_amd._lib import MAX_WS_TAG
from edgegaussians_amd.journal import (WINDOW_TAGS, Batched, DataParallel, EpochMark, Regulariser, StepJournal, Steps,
                                       chunks)
from edgegaussians_amd.trainer import EdgeTrainer


class HostTrainer(EdgeTrainer):
    """EdgeTrainer's prologue, entry points and journal over recording stand-ins of every device operation."""

    def __init__(self, replay_on_overflow=True):
        self._journal = StepJournal(self)
        self.replay_on_overflow = replay_on_overflow
        self.capacity, self.epoch, self.loss_scale = 1, 0, 1.0
        self._loss_buf = torch.zeros(65)
        self.loss_acc, self._n_marks = self._loss_buf[:1], 0
        self.log = []
        self.most = 0  # the longest journal seen

    def _bind_stream(self):
        pass

    def _snapshot(self):
        self.log.append(("snapshot", len(self._journal)))
        self.snap = (self.epoch, self.loss_scale)

    def _restore(self):
        self.log.append(("restore",))
        self.epoch, self.loss_scale = self.snap

    def flush(self):
        if self._journal:
            self.log.append(("flush", len(self._journal)))
            self._journal.clear()

    def _zero_workspaces(self):
        self.log.append(("zero", self._journal.tag))

    def _ctl_bits(self):
        return False, False

    def _steps_raw(self, views, wmaps):
        self.most = max(self.most, len(self._journal))
        self.log.append(("run", len(views), self._journal.take(len(views))))

    def _step_raw(self, view, wmap):
        self.log.append(("step", view, self.epoch, self.loss_scale, self._journal.take(1)))

    def _batched_raw(self, views, wmaps, fused_adam, *a):
        self.log.append(("batched", list(views), self.epoch, self.loss_scale, self._journal.take(1)))

    def _regulariser_raw(self, kind, avg_loss_sum, *settings):
        self.log.append(("reg", kind, self.epoch, self.loss_scale))

    def _mark_raw(self, k):
        self.log.append(("mark", k, self.epoch, self.loss_scale))


def test_tag_cost_of_each_entry_kind():
    assert Steps([0, 1, 2], [None] * 3).tags == 3
    assert Batched([0, 1, 2], [None] * 3).tags == 1
    assert Regulariser("direction", 0.01, 5, "enforce_full").tags == 0
    assert EpochMark(0).tags == 0
    assert DataParallel([0, 1], [None] * 2, [1, None]).tags == 2       # one grad_step per view
    assert DataParallel([[0, 1]], [[None, None]], [None]).tags == 2   # two half batches
    # ... and what the entry points draw: exactly the declared tags
    tr = HostTrainer()
    tr.train_steps([0, 1, 2], [None] * 3)
    assert tr._journal.tag == 3
    tr.train_step(0, None)
    tr.train_step_batched([0, 1], [None, None])
    assert tr._journal.tag == 5
    tr.regulariser_step("ratio", want_value=False)
    tr.mark_epoch()
    assert tr._journal.tag == 5 and len(tr._journal) == 3 + 1 + 1 + 1 + 1


def test_a_run_longer_than_a_window_is_chunked_and_read_back_in_between():
    tr = HostTrainer()
    K = MAX_WS_TAG // 2 + 100
    tr.train_steps(list(range(K)), [None] * K)
    assert WINDOW_TAGS == MAX_WS_TAG // 2
    assert tr.log == [("snapshot", 0), ("run", WINDOW_TAGS, 1), ("flush", WINDOW_TAGS),
                      ("snapshot", 0), ("run", 100, WINDOW_TAGS + 1)]
    assert tr.most <= MAX_WS_TAG // 2 and len(tr._journal) == 100
    assert [len(c[0]) for c in chunks(list(range(K)), [None] * K)] == [WINDOW_TAGS, 100]


def test_the_window_is_read_back_before_its_replay_could_run_out_of_tags():
    tr = HostTrainer()
    tr.train_steps(list(range(WINDOW_TAGS - 1)), [None] * (WINDOW_TAGS - 1))
    tr.train_step_batched([0, 1], [None, None])   # exactly fills the window
    assert not [x for x in tr.log if x[0] == "flush"]
    tr.train_step(0, None)                        # would pass it
    assert ("flush", WINDOW_TAGS) in tr.log and len(tr._journal) == 1


def test_the_wrap_zeroes_the_workspaces_exactly_when_the_range_would_be_passed():
    for replay in (True, False):
        tr = HostTrainer(replay_on_overflow=replay)
        tr._journal.tag = MAX_WS_TAG - 4
        tr.train_steps([0, 1, 2, 3], [None] * 4)  # the last four tags of the range
        assert tr._journal.tag == MAX_WS_TAG and not [x for x in tr.log if x[0] == "zero"]
        tr.train_step(0, None)                    # one more would pass MAX_WS_TAG
        zeros = [i for i, x in enumerate(tr.log) if x[0] == "zero"]
        assert len(zeros) == 1 and tr._journal.tag == 1
        flushes = [i for i, x in enumerate(tr.log) if x[0] == "flush"]
        # the window's sticky words are read before they are zeroed (and an empty journal has nothing to read)
        assert flushes == ([zeros[0] - 1] if replay else [])


def test_the_snapshot_is_taken_for_the_first_entry_of_a_window_only():
    tr = HostTrainer()
    tr.train_step(0, None)
    tr.train_steps([1, 2], [None, None])
    tr.regulariser_step("direction", want_value=False)
    tr.train_step_batched([0, 1], [None, None])
    assert [x for x in tr.log if x[0] == "snapshot"] == [("snapshot", 0)]
    tr.flush()
    tr.train_step(0, None)
    assert [x for x in tr.log if x[0] == "snapshot"] == [("snapshot", 0)] * 2
    off = HostTrainer(replay_on_overflow=False)
    off.train_steps([0, 1], [None, None])
    assert not off._journal and not [x for x in off.log if x[0] == "snapshot"]


def test_mark_epoch_is_journalled_inside_a_window_only():
    tr = HostTrainer()
    assert tr.mark_epoch() == 0
    assert len(tr._journal) == 0 and not [x for x in tr.log if x[0] == "snapshot"]
    tr.train_step(0, None)
    assert tr.mark_epoch() == 1
    assert [type(e) for e in tr._journal.entries] == [Steps, EpochMark] and tr._journal.entries[1].k == 1


def test_replay_runs_the_entries_in_order_with_their_epoch_and_loss_scale():
    tr = HostTrainer()
    tr.epoch, tr.loss_scale = 3, 0.5
    tr.train_steps([0, 1], [None, None])
    tr.regulariser_step("direction", want_value=False)
    tr.mark_epoch()
    tr.epoch, tr.loss_scale = 4, 0.25
    tr.train_step_batched([2, 0], [None, None])
    tr.train_step(1, None)
    tr.epoch, tr.loss_scale = 5, 0.125  # (the current ones: set after the last enqueue)
    tr.log.clear()
    tag = tr._journal.tag
    tr._journal.replay()
    assert [x[:4] if x[0] != "restore" else x for x in tr.log] == [
        ("restore",), ("step", 0, 3, 0.5), ("step", 1, 3, 0.5), ("reg", "direction", 3, 0.5), ("mark", 0, 3, 0.5),
        ("batched", [2, 0], 4, 0.25), ("step", 1, 4, 0.25)]
    assert (tr.epoch, tr.loss_scale) == (5, 0.125) and len(tr._journal) == 6
    assert tr._journal.tag == tag + 4  # fresh tags for the replayed forwards


def test_replay_wraps_the_tags_up_front_when_the_window_would_pass_the_range():
    tr = HostTrainer()
    tr._journal.tag = MAX_WS_TAG - 10
    tr.train_steps([0, 1, 2, 3, 4, 5], [None] * 6)
    tr.log.clear()
    tr._journal.replay()
    assert tr.log[0] == ("zero", MAX_WS_TAG - 4) and tr._journal.tag == 6
