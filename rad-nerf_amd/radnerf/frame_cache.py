"""What the fused inference engine (radnerf/fused.py) builds once and reuses across frames, free of the HIP library and of any
device: the record of one built artifact, the slot that decides when one is built, kept and dropped, the per-model owner of the
slots and of the per-stream states, and the lazily read loop statistics.  Streams, events and tensors are the caller's:
tests/test_frame_cache_host.py drives all of it with stand-ins.

THE RULE (Slot.get), for every artifact that is built from inputs named by a key: a held record whose key differs is dropped,
and that call gets nothing; the first sight of a key only remembers it, with the tensors it names; a key seen on the call before
is built; a build that yields nothing is held like any other, so it is not tried again on every frame, and its readers get
nothing.  A caller whose key moves or alternates with every call (patch batches, validation frames between training steps)
therefore never pays for a build.  Nothing is ever built under stream capture."""
import collections.abc


class Built:
    """One built artifact: `key` names what it was built from, `refs` keeps those tensors alive (none of their addresses can be
    handed to another tensor, and come back as a false match, while the record lives), `tensors` are the device buffers a reader
    uses (none: the build yielded nothing), `event` was recorded behind the build on `stream` (its handle), `waited` are the
    handles of the streams ordered behind the build so far.  Whatever else the owner names (n_on, gx, levels, ...) is an attribute."""

    def __init__(self, key, refs, tensors, event, stream, **payload):
        self.key, self.refs, self.tensors, self.event, self.waited = key, refs, tuple(tensors), event, {stream}
        self.__dict__.update(payload)

    def order(self, stream):
        """Order `stream` behind the build, once: it waits for the event, and the allocator hears of its use of every tensor."""
        if stream.cuda_stream not in self.waited:
            stream.wait_event(self.event)
            for t in self.tensors:
                t.record_stream(stream)
            self.waited.add(stream.cuda_stream)


class Slot:
    """At most one Built, by THE RULE above.  `held` is the record, `seen` the (key, refs) of the last call that found none,
    `builds` counts the records made (record(), which every builder returns through).

    `use_under_capture`: may a held record be handed out on a capturing stream?  False -- the dense image of the xyz table --
    leaves the slot untouched by such a call, `seen` included: a replayed graph would go on reading an image the table has
    moved away from.  True -- the torso plan -- hands a held plan out and still never builds (rn_torso_plan_build reads a count
    back and refuses a capturing stream); why a replay may read a plan its grid has moved away from is written nowhere in the
    history: the value is kept as found."""

    def __init__(self, use_under_capture):
        self.use_under_capture, self.builds = use_under_capture, 0
        self.forget()

    def forget(self):
        self.held = self.seen = None

    def record(self, key, refs, tensors, event, stream, **payload):
        self.builds += 1
        return Built(key, refs, tensors, event, stream, **payload)

    def get(self, key, refs, build, capturing=False):
        """The held record of `key`, or None; build() -> Built is called where THE RULE says so."""
        if capturing and not self.use_under_capture:
            return None
        if self.held is not None and self.held.key != key:
            self.held = None
        if self.held is None:
            if self.seen is None or self.seen[0] != key:
                self.seen = (key, refs)
                return None
            if capturing:
                return None
            self.held = build()
        return self.held if self.held.tensors else None


class FrameCaches:
    """What one model's fused engine keeps between frames: `states`, stream handle -> its FusedState (a renderer that keeps two
    frames in flight uses two streams, and each needs its own loop state and scratch); `loop_hint` (fused.set_loop_hint); the
    slots of the torso plan and of the dense image, shared by the streams.  copy.deepcopy(model) does not carry it over: the
    copy starts empty."""

    def __init__(self):
        self.states, self.loop_hint, self.plan, self.image = {}, None, Slot(use_under_capture=True), Slot(use_under_capture=False)

    def __deepcopy__(self, memo):
        return type(self)()


class LoopStats(collections.abc.Mapping):
    """Loop statistics of the frame just enqueued: st.read_loop_stats() -> dict, called once, at the first access (which
    synchronises the stream)."""

    def __init__(self, st):
        self._st, self._read = st, None

    def _load(self):
        if self._read is None:
            self._read = self._st.read_loop_stats()
        return self._read

    def __getitem__(self, k):
        return self._load()[k]

    def __iter__(self):
        return iter(self._load())

    def __len__(self):
        return len(self._load())

    def __repr__(self):
        return repr(self._load())
