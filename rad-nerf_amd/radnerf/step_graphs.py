"""What GraphedTrainer (radnerf/train.py) keeps between captured steps, free of the HIP library and of any device: a device scalar
that is refilled only when its host value moved, the static inputs a captured step reads, and the bounded least-recently-used
cache of captured graphs over such inputs.  The capture itself is the caller's (tests/test_step_graphs_host.py drives all three
with CPU tensors and stand-in graphs)."""
import torch


class HeldScalar:
    """A device tensor of one element and the host value it was last filled with: set(value) launches a fill only when the value
    moved (the sample budget moves every 16 steps, the ambient weight is constant once its ramp is over)."""

    def __init__(self, shape, dtype, device):
        self.tensor, self.value = torch.zeros(shape, dtype=dtype, device=device), None

    def set(self, value):
        if value != self.value:
            self.tensor.fill_(value)
            self.value = value
        return self.tensor


class StaticInputs:
    """The static inputs of one ray layout: `static`, clones of a batch's tensors for a graph to read, with the frame index as a
    device tensor; `index`, the frame index list they currently hold; `budget`, None or the layout's own sample budget
    (device int32, rows, True) -- True: it covers every row of every ray (a patch layout)."""

    def __init__(self, data, device, budget=None):
        if "_packed" in data:        # a batch that is one table of rows: one static tensor, the step's inputs are its views
            static = dict(data["_unpack"](data["_packed"].clone()))
        else:
            static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}
        self.index = None
        if isinstance(static.get("index"), (list, tuple)):     # a Python list would be uploaded inside the capture
            self.index = list(static["index"])
            static["index"] = torch.tensor(static["index"], dtype=torch.long, device=device)
        self.static, self.budget = static, budget

    def feed(self, data):
        """Copy a batch into the static inputs."""
        static = self.static
        if "_packed" in data and "_packed" in static:
            static["_packed"].copy_(data["_packed"])
            for k in ("poses", "eye", "auds"):
                if data[k] is not static[k]:
                    static[k].copy_(data[k])
        else:
            for k, v in data.items():
                if torch.is_tensor(v) and k != "_packed":
                    static[k].copy_(v)
        v = data.get("index")
        if isinstance(v, (list, tuple)) and list(v) != self.index:
            # a feed whose frame changes every step brings the index as a device tensor too (DeviceTrainSet): a copy on the
            # stream instead of an upload from pageable memory, which the host waits for
            src = data.get("_index_dev")
            static["index"].copy_(src if src is not None else torch.tensor(v, dtype=torch.long))
            self.index = list(v)


class GraphCache:
    """At most `bound` captured steps, least recently used first: `graphs` maps key -> (graph, loss, layout), `inputs` maps
    layout -> the StaticInputs that layout's graphs share (several keys -- row capacities -- of one ray layout read one set)."""

    def __init__(self, bound):
        self.bound, self.graphs, self.inputs = int(bound), {}, {}

    def get(self, key, layout, capture):
        """-> (graph, loss, static inputs) of `key`, most recently used from now on.  On a miss capture(inputs) -> (graph, loss,
        inputs) records the step, given the layout's static inputs or None where no held graph has that layout; then the least
        recently used entries beyond the bound go -- never the newest -- each taking its layout's static inputs with it when no
        other graph reads them."""
        entry = self.graphs.pop(key, None)
        if entry is None:
            graph, loss, self.inputs[layout] = capture(self.inputs.get(layout))
            entry = (graph, loss, layout)
        self.graphs[key] = entry                               # dicts keep insertion order: the last entry is the most recent
        while len(self.graphs) > max(self.bound, 1):
            gone = self.graphs.pop(next(iter(self.graphs)))[2]
            if not any(e[2] == gone for e in self.graphs.values()):
                del self.inputs[gone]
        return entry[0], entry[1], self.inputs[layout]

    def newest(self):
        """(graph, loss, static inputs) of the most recently used entry."""
        graph, loss, layout = next(reversed(self.graphs.values()))
        return graph, loss, self.inputs[layout]
