"""Stream discipline of the backward sweep's side-work scheduler (mafed_amd.engine.SideWork), driven with stub streams: no GPU."""
import contextlib

from mafed_amd.engine import SideWork


class Event:
    def __init__(self, stream):
        self.stream = stream


class Stream:
    """Counts its calls and writes each into ``timeline``, the one list (shared with the work of Rig.work) that orders waits against work."""

    def __init__(self, name, timeline):
        self.name, self.timeline, self.recorded, self.waited_events, self.waited_streams = name, timeline, [], [], []

    def record_event(self):
        self.recorded.append(Event(self))
        self.timeline.append(("record", self.name, self.recorded[-1]))
        return self.recorded[-1]

    def wait_event(self, ev):
        self.waited_events.append(ev)
        self.timeline.append(("wait", self.name, ev))

    def wait_stream(self, st):
        self.waited_streams.append(st)
        self.timeline.append(("wait_stream", self.name, st))


class Rig:
    """A scheduler over one main and ``n_side`` side stubs; ``work(tag)`` makes a hand-off that logs (tag, the stream current when it ran)
    and writes ("work", that stream, tag) into the timeline."""

    def __init__(self, n_side):
        self.timeline = []
        self.main = Stream("main", self.timeline)
        self.sides = [Stream(f"side{k}", self.timeline) for k in range(n_side)] if n_side else None
        self.current, self.log = [self.main], []
        self.sched = SideWork(self.main, self.sides, enter=self.enter)

    @contextlib.contextmanager
    def enter(self, stream):
        self.current.append(stream)
        try:
            yield
        finally:
            self.current.pop()

    def work(self, tag):
        def run():
            self.log.append((tag, self.current[-1].name))
            self.timeline.append(("work", self.current[-1].name, tag))
        return run

    def at(self, *entry):
        return self.timeline.index(entry)


def test_consecutive_handoffs_share_one_event():
    r = Rig(3)
    for tag in "abc":
        r.sched.on_side(r.work(tag))
    assert len(r.main.recorded) == 1
    ev = r.main.recorded[0]
    assert [s.waited_events for s in r.sides] == [[ev], [ev], [ev]]
    # the event is recorded, then each side stream waits for it, then -- and only then -- its work runs there
    assert r.timeline == [("record", "main", ev)] + [e for k, tag in enumerate("abc") for e in (("wait", f"side{k}", ev), ("work", f"side{k}", tag))]


def test_main_moved_between_handoffs_records_a_second_event():
    r = Rig(3)
    r.sched.on_side(r.work("a"))
    r.sched.main_moved()
    r.sched.on_side(r.work("b"))
    r.sched.on_side(r.work("c"))
    first, second = r.main.recorded
    assert r.sides[0].waited_events == [first] and r.sides[1].waited_events == [second] and r.sides[2].waited_events == [second]
    # the second event is recorded after the main stream moved, and each hand-off waits for its event before it works
    assert r.at("work", "side0", "a") < r.at("record", "main", second) < r.at("wait", "side1", second) < r.at("work", "side1", "b")
    assert r.at("wait", "side0", first) < r.at("work", "side0", "a") and r.at("wait", "side2", second) < r.at("work", "side2", "c")


def test_without_side_streams_work_runs_inline_and_records_nothing():
    r = Rig(0)
    kept = object()
    r.sched.on_side(r.work("a"), kept)
    r.sched.after_all(r.work("hook"))
    r.sched.join()
    assert r.log == [("a", "main"), ("hook", "main")]
    assert r.main.recorded == [] and r.main.waited_events == [] and r.main.waited_streams == []
    assert r.sched.keep == []   # inline work has finished with its tensors: nothing is kept


def test_handoffs_rotate_over_the_side_streams_in_order():
    r = Rig(3)
    for i in range(7):
        r.sched.on_side(r.work(i))
    assert r.log == [(i, f"side{i % 3}") for i in range(7)]
    r.sched.on_side(r.work("pinned"), k=2)   # an explicit index neither follows nor advances the rotation
    r.sched.on_side(r.work(7))
    assert r.log[-2:] == [("pinned", "side2"), (7, "side1")]


def test_bucket_hook_runs_on_side_0_behind_every_other_side_stream():
    r = Rig(3)
    r.sched.on_side(r.work("a"))
    r.sched.on_side(r.work("b"))
    r.sched.after_all(r.work("hook"))
    assert r.log[-1] == ("hook", "side0")
    assert [len(s.recorded) for s in r.sides] == [0, 1, 1]   # one event from each other side stream
    main_ev = r.main.recorded[0]   # (the hook is a hand-off like any other: it shares the main stream's current event)
    assert len(r.main.recorded) == 1
    e1, e2 = r.sides[1].recorded[0], r.sides[2].recorded[0]
    assert r.sides[0].waited_events == [main_ev, main_ev, e1, e2]
    # the other streams' events are recorded behind the work queued on them, and side 0 has waited for the main stream's event and for
    # both of them when the hook enters
    assert r.at("work", "side1", "b") < r.at("record", "side1", e1) and r.at("record", "side1", e1) < r.at("wait", "side0", e1)
    assert r.timeline[-4:] == [("wait", "side0", main_ev), ("wait", "side0", e1), ("wait", "side0", e2), ("work", "side0", "hook")]
    # the hook does not advance the rotation either: the next hand-off goes where it would have gone
    r.sched.on_side(r.work("c"))
    assert r.log[-1] == ("c", "side2")


def test_join_waits_for_every_side_stream_once_and_drops_the_kept_tensors():
    r = Rig(3)
    a, b = object(), object()
    r.sched.on_side(r.work("a"), a, b)
    r.sched.on_side(r.work("b"), b)
    assert r.sched.keep == [a, b, b]
    r.sched.join()
    assert r.main.waited_streams == r.sides
    assert r.timeline[-3:] == [("wait_stream", "main", st) for st in r.sides]   # after everything handed off
    assert r.sched.keep == []
    assert all(s.waited_streams == [] for s in r.sides)
