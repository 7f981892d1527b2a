"""
Online (chunk-by-chunk) separation of a CAUSAL Conv-TasNet: audio goes in as it arrives, separated audio comes out L - S samples later.

    sep = model.online_separator(num_streams=64, chunk_size=80)
    for chunk in chunks:                 # (num_streams, 1, k S) on the model's device
        y = sep(chunk)                   # (num_streams, n_sources, k S)
    tail = sep.flush()                   # (num_streams, n_sources, L - S), then every stream starts over

Contract (L = kernel_size, S = stride): a stream starts with L - S zero samples of pre-roll; every chunk of n S samples yields n encoder frames
and exactly n S output samples per source; flush() returns the last L - S samples.  For a mono input x of length m (a multiple of S)

    torch.cat([sep(c) for c in chunks] + [sep.flush()], -1) == model(F.pad(x, (L - S, 0)))

and the separated version of x[t] is output sample t + L - S (algorithmic delay L - S samples).  It holds because a causal model's mask frame f
depends on encoder frames <= f only -- cLN is cumulative (reference src/modules/norm.py:42-101), the depthwise taps are left-padded by (P - 1) d
(src/models/tdcn.py:125-132) -- and output sample tau receives overlap-add from the frames f with f S <= tau < f S + L only.  The same holds
for the causal family with separable=False (two full P-tap convolutions per layer, left-padded alike): per layer the pass is conv1, cLN,
sep_online_unfold_fwd (the depthwise kernel's history, no taps: rows c P + p of an (H P, ldt) buffer), and the heads' products over those rows.

A chunk step is net.py-style orchestration: backend calls only, no autograd and no torch kernel between the launches of a chunk.  Every stream's
n frames are columns stream * n + frame of one (C, ldt) matrix ("stream-major"), so each 1x1 product of a layer is ONE sep_pw_gemm over all
streams; the state that carries from chunk to chunk (encoder carry, frame counters, the cLN running sums, the depthwise histories, the
overlap-add tail) lives in device memory and is read by the kernels of csrc/online.hip.  The first chunk of `chunk_size` samples is recorded
(sepkernels.recording) and later chunks of that size replay it with one sep_run_sequence call; other sizes run the same launches eagerly.
Every call, whichever of the forms below it takes, goes through one path (OnlineSeparator._call: check, workspace, upload, record or replay,
clone) on one workspace per chunk width.  No gradients: training is out of scope.

Streams on their own clocks.  A separator is a set of `num_streams` SLOTS; sep(chunk, streams=...) advances only the slots it names and
flush(streams) / reset(streams) end / restart only those, so the contract above holds PER STREAM whichever other streams took part in which
calls and however long a stream sat idle:

    y = sep(chunk, streams=[7, 2])       # chunk (2, 1, k S): row 0 is slot 7's audio, row 1 slot 2's -> (2, n_sources, k S), same order
    tail = sep.flush([7])                # (1, n_sources, L - S); slot 7 starts over, every other slot is untouched

    torch.cat(pieces slot s received + [sep.flush([s])], -1) == model(F.pad(x_s, (L - S, 0)))

`streams` is a list of indices in any order, an integer tensor, or a bool mask of num_streams entries (selects in ascending order); duplicates,
indices out of range, an empty selection and a chunk whose rows do not match the selection are ValueErrors.  All streams of one call share one
chunk length.  The pass of a subset call runs over the A selected streams only -- A n stream-major columns, T = A n in every product, A
workgroups (or rows of workgroups) in the state kernels, the sep_online_*_sel entry points -- so idle slots cost their memory and nothing
else.  The slot list lives in a device buffer of the workspace that is filled before every call like the chunk, so a step recorded for (A, n)
replays for ANY selection of A slots.  One workspace per chunk length serves every A and the all-streams call: a pass's matrices are laid out
with the leading dimension round_up(A n, 128) inside storage sized for all slots, and a recording per A holds a launch list only.  At most `max_recordings` (default 8)
of them are kept, the least recently used one is dropped first -- a recording owns no device memory of its own, so dropping one is safe at
any time and the next call of that A records again.  streams=None is the all-streams call: it issues exactly the launches it always did, and
its recording is kept apart from those -- not counted against `max_recordings`, never dropped for one of them.  When model.to() has replaced
the flat parameter buffer the recordings were made under, all of them are dropped and made again.

Ragged calls.  With `lengths` every stream of a call brings its own number of samples, so one pass carries whatever each stream has right now:

    y = sep(chunk, streams=[7, 2, 5], lengths=[80, 8, 24])   # chunk (3, 1, W), W a multiple of S; lengths in samples
    ys = sep([x7, x2, x5], streams=[7, 2, 5])                # a list of (1, k_j S) or (k_j S,) tensors -> a list of (n_sources, k_j S)

`lengths` has one entry per row (a list, or an integer tensor on any device), each a positive multiple of S and <= W.  Row j's samples beyond
lengths[j] are ignored, the result is (A, n_sources, W) with row j zero beyond lengths[j], and slot streams[j] advances by lengths[j] / S frames.
streams=None with `lengths` of num_streams entries is the all-streams ragged call.  The list form pads on the device to the longest piece and
calls the tensor form.  The per-stream contract is unchanged, whatever lengths a slot and the others brought to which calls; flush and reset
are untouched.  A wrong count of lengths, a length that is zero, negative, not a multiple of S or > W, and a non-integer tensor are ValueErrors
that leave no trace in the state.  With lengths=None a call issues exactly the launches it did before; with `lengths` the ragged path always
runs, even if all entries are equal.  The columns of a ragged pass are compact: block j is [offs[j], offs[j + 1]) with offs the running sum of
the frame counts, ldt = round_up(offs[A], 128), and offs sits in a device buffer next to the slot list that is filled before every call (the
sep_online_*_rag entry points read it when they run).  The step is the launch list of a subset step; its products run over T = ldt columns --
the dead columns [offs[A], ldt) are zero wherever a state kernel wrote, only ever feed themselves, and no state kernel nor the decoder reads
them -- so the launch arguments depend on (A, ldt, W) only: a ragged call with W == chunk_size is recorded per (A, ldt) and replayed for ANY
lengths with that total, under the same `max_recordings` bound.  Other widths run eagerly.

State that travels.  Everything a slot carries from call to call can leave the separator it started in and come back, for some slots while the
others keep running:

    state = sep.export_state([3, 1])     # OnlineState: row 0 is slot 3, row 1 slot 1; the separator is not changed
    other.import_state(state[0], [1])    # slot 1 of ANOTHER separator of the same model structure goes on where slot 3 was (migration)
    torch.save(state.cpu().state_dict(), f);  state = OnlineState.from_state_dict(torch.load(f))       # tensors and builtin values only
    sep.import_state(state, [3, 1])      # back to the moment of the export: the same calls then give the same bits again (rollback)

A state is one (A, row_bytes) uint8 tensor -- one packed row per slot, written and read by ONE launch each (sep_online_state_export /
sep_online_state_import, the row format is documented in include/sepkernels.h as version 1) -- plus a header of plain Python values that
import_state compares with its own separator before anything is uploaded.  Import writes into the existing state buffers in place, so every
recorded step stays valid.  An imported slot behaves exactly as the exported one would have; flush, reset, subset and ragged calls are
unchanged.  Whether the WEIGHTS are the same cannot be checked cheaply and is not checked.
"""
import collections
import itertools
import types

import torch

import sepkernels
from . import backend, EPI_SIGMOID, PRO_PRELU
from . import functional as _fn


def _round_up(a, b):
    return (a + b - 1) // b * b


class _Workspace:
    """the activations of every call of one chunk width (n frames per row): storage for all slots, handed out as the (C, ldt) stream-major
    matrices of one pass.  Passes of different ldt share the storage, so a pass finds another's leftovers in its dead columns: every kernel
    of a pass that writes a matrix zeroes its own columns [T, ldt), and a column of a product depends on that column alone"""

    def __init__(self, sep, n):
        f = dict(device=sep.device, dtype=sep.dtype)
        Bs = sep.num_streams
        self.n = n
        ldt = _round_up(Bs * n, 128)
        self.chunk = torch.zeros(Bs, n * sep.S, **f)
        self.out = torch.zeros(Bs, sep.n_src, n * sep.S, **f)
        self.slots = torch.zeros(Bs, device=sep.device, dtype=torch.int32)        # calls on a selection: the slot of every row
        self.offs = torch.zeros(Bs + 1, device=sep.device, dtype=torch.int32)     # ragged calls: the column block of every row
        self.amax = torch.zeros(1, **f)
        self.rows = dict(w=sep.N, wn=sep.N, xa=sep.Bn, xb=sep.Bn, ha=sep.H, hb=sep.H, total=sep.Sc, m=sep.n_src * sep.N)
        if sep.dense:                                          # separable=False: the normalised activation unfolded over the taps, rows c P + p
            self.rows["cols"] = sep.H * sep.P
        self.store = {k: torch.zeros(C * ldt, **f) for k, C in self.rows.items()}
        self.cache = {}                                        # (blocks, ldt) -> views: a stream of calls asks for the same few again and again

    def views(self, blocks, ldt=None):
        """-> what _step takes: the rows of chunk and out and the matrices of a pass over `blocks` column blocks.  ldt: of a ragged call
        (round_up of the frames it carries, 128); None: of a call whose blocks bring n frames each, round_up(blocks n, 128)"""
        ldt = _round_up(blocks * self.n, 128) if ldt is None else ldt
        v = self.cache.get((blocks, ldt))
        if v is None:
            if len(self.cache) >= 256:                         # views own no memory: forgetting them costs the next calls their making, no more
                self.cache.clear()
            v = self.cache[blocks, ldt] = types.SimpleNamespace(ldt=ldt, chunk=self.chunk[:blocks], out=self.out[:blocks], amax=self.amax)
            for k, C in self.rows.items():
                setattr(v, k, self.store[k][:C * ldt].view(C, ldt))
            v.block = {id(m): m.unsqueeze(0) for m in (getattr(v, k) for k in self.rows)}  # id(matrix) -> it as one (1, C, ldt) block of all streams
        return v


STATE_FORMAT_VERSION = 1                                   # the row format of include/sepkernels.h ("export / import of the online separator's per-stream state")
_HEADER_KEYS = ("version", "L", "S", "n_sources", "n_norms", "ring_len", "separable", "config", "dtype")


class OnlineState:
    """The state of A slots of an OnlineSeparator, taken by export_state: `blob`, an (A, row_bytes) uint8 tensor with one packed row per slot
    (row format `version`, include/sepkernels.h), and a header of plain Python values that says which separators can take it -- `version`,
    `L`, `S`, `n_sources`, `n_norms`, `ring_len`, `separable`, `config` (the model's get_config()) and `dtype` (a string).  It owns its
    blob: nothing in it refers to the separator it came from.

    len(state)              the number of rows
    state.frames            (A,) int64, the frame counter of every row, decoded from the blob on request (on the blob's device)
    state.to(device), state.cpu()
    state[i], state.select(rows)    a state of the chosen rows (an index, a slice, or a list / tensor of indices), in that order
    state.state_dict(), OnlineState.from_state_dict(d)      a dict of one tensor and builtin values: it survives torch.save / torch.load"""

    def __init__(self, blob, header):
        missing = [k for k in _HEADER_KEYS if k not in header]
        if missing:
            raise ValueError("an online state's header lacks {}".format(missing))
        if not torch.is_tensor(blob):
            raise ValueError("an online state's blob is a tensor (got {})".format(type(blob).__name__))
        self.blob = blob
        self.header = {k: header[k] for k in _HEADER_KEYS}

    def __getattr__(self, name):                               # state.version, state.L, ... : the header's entries
        header = self.__dict__.get("header")
        if header is not None and name in header:
            return header[name]
        raise AttributeError(name)

    def __len__(self):
        return self.blob.shape[0]

    @property
    def frames(self):
        if self.blob.dim() != 2 or self.blob.dtype != torch.uint8 or self.blob.shape[1] < 8:
            raise ValueError("the blob is not a (rows, row_bytes) uint8 tensor: it holds no frame counters")
        return self.blob[:, :8].contiguous().view(torch.int64).reshape(-1)

    def to(self, device):
        return OnlineState(self.blob.to(device), self.header)

    def cpu(self):
        return self.to("cpu")

    def select(self, rows):
        if torch.is_tensor(rows):
            rows = rows.reshape(-1).tolist()
        rows = [int(r) for r in rows]
        if any(r < -len(self) or r >= len(self) for r in rows):
            raise IndexError("row out of range: the state has {} rows".format(len(self)))
        return OnlineState(self.blob[[r % len(self) for r in rows]] if rows else self.blob[:0].clone(), self.header)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.select(list(range(len(self)))[i])
        if isinstance(i, int):
            return self.select([i])
        return self.select(i)

    def state_dict(self):
        d = {"format_version" if k == "version" else k: (dict(v) if k == "config" else v) for k, v in self.header.items()}
        d["blob"] = self.blob
        return d

    @classmethod
    def from_state_dict(cls, d):
        header = dict(d)
        blob = header.pop("blob", None)
        if "format_version" in header:
            header["version"] = header.pop("format_version")
        return cls(blob, header)


class OnlineSeparator:
    """Chunk-by-chunk separation of `num_streams` independent mono streams by a causal Conv-TasNet (see the module docstring for the contract).
    Built by ConvTasNet.online_separator; reads the model's live parameters at every chunk (an in-place update or load_state_dict is seen at
    the next chunk; after model.to() moved the flat parameter buffer the recording is dropped and made again).

    delay        L - S: output sample t + delay is the separated version of input sample t
    state_bytes  device memory of the per-stream state (carry, frame counter, cLN sums, depthwise histories, overlap-add tail)

    max_recordings  how many recorded subset steps (one per number of selected streams A, at `chunk_size`) and ragged steps (one per (A, ldt)) are
                    kept; the least recently used one is dropped first and recorded again when that A or (A, ldt) comes back"""

    def __init__(self, model, num_streams=1, chunk_size=None, record=True, max_recordings=8):
        if not model.causal:
            raise ValueError("online separation needs a causal model: gLN (causal=False) normalises over the whole signal, which has not arrived yet")
        if not model.staged:
            raise NotImplementedError("online separation runs the staged causal family only; this model is outside it: {}".format(model.staged_reason))
        if model.in_channels != 1:
            raise NotImplementedError("online separation takes mono streams (in_channels=1), the model has in_channels={}".format(model.in_channels))
        if num_streams < 1:
            raise ValueError("num_streams must be >= 1")
        if max_recordings < 1:
            raise ValueError("max_recordings must be >= 1")
        K = backend()
        flat = model.flat_parameters()
        if flat is None:
            raise RuntimeError("online separation needs the model's parameters co-located in its flat buffer")
        if K.name == "hip" and (not flat.is_cuda or flat.dtype != torch.float32):
            raise RuntimeError("online separation runs on the GPU in fp32: move the model to 'cuda' (parameters are {} {})".format(flat.device, flat.dtype))
        self.model = model
        self.device, self.dtype = flat.device, flat.dtype
        self.num_streams = num_streams
        self.L, self.S = model.kernel_size, model.stride
        self.delay = self.L - self.S
        if chunk_size is not None and (chunk_size <= 0 or chunk_size % self.S):
            raise ValueError("chunk_size must be a positive multiple of the stride {} (got {})".format(self.S, chunk_size))
        self.chunk_size = chunk_size
        self.record = bool(record) and getattr(K, "records", False)
        sep = model.separator
        self.N, self.n_src = model.n_basis, model.n_sources
        self.Bn, self.Sc = model.sep_bottleneck_channels, model.sep_skip_channels
        self.H = model.sep_hidden_channels
        self.layers = [layer for block in sep.tdcn.net for layer in block.net]
        self.dense = not model.separable                       # full P-tap convolutions: one norm per layer, the taps by the online unfold
        self.P = model.sep_kernel_size
        self.n_norms = 1 + (1 if self.dense else 2) * len(self.layers)
        self.ring_offsets, off = [], 0
        for layer in self.layers:                              # (C, (P - 1) d) per layer: the depthwise input's history, or the unfold's
            self.ring_offsets.append(off)
            off += self.H * (layer.kernel_size - 1) * layer.dilation
        self.ring_len = off
        f = dict(device=self.device, dtype=self.dtype)
        Bs, keep = num_streams, self.delay
        self.frames = torch.zeros(Bs, device=self.device, dtype=torch.int64)
        self.carry, self.carry_next = torch.zeros(Bs, keep, **f), torch.zeros(Bs, keep, **f)
        self.sums = torch.zeros(Bs, 2 * self.n_norms, device=self.device, dtype=torch.float64)
        self.rings = torch.zeros(Bs, self.ring_len, **f)
        self.tail, self.tail_next = torch.zeros(Bs, self.n_src, keep, **f), torch.zeros(Bs, self.n_src, keep, **f)
        self.state_bytes = sum(t.numel() * t.element_size() for t in (self.frames, self.carry, self.carry_next, self.sums, self.rings, self.tail,
                                                                       self.tail_next))
        self.max_recordings = int(max_recordings)
        self._ws = {}                                          # chunk width in hops (ragged calls: the row pitch) -> _Workspace, for every call form
        self._seq = None                                       # the all-streams step at chunk_size: apart from the bound and the eviction of the others
        self._sub_seqs = collections.OrderedDict()             # A (subset step) or (A, ldt) (ragged step) -> Sequence at chunk_size, least recently used first
        self.replays = collections.Counter()                   # ragged recording key -> how often it was replayed
        self._flat = None                                      # the model's flat parameter buffer the recordings were made under
        self._state_slots = None                               # export_state / import_state: the slot list on the device, filled before every call

    # ------------------------------------------------------------------ public
    def __call__(self, chunk, streams=None, lengths=None):
        """chunk (num_streams, 1, k S) -> (num_streams, n_sources, k S); with `streams` (indices in any order, an integer tensor or a bool mask)
        chunk is (A, 1, k S) for the A selected streams in that order, only they advance, and the result is (A, n_sources, k S).  With `lengths`
        (samples per row, positive multiples of S, <= k S) row j brings lengths[j] samples, advances by lengths[j] / S frames and comes back zero
        beyond lengths[j]; a list of (1, k_j S) or (k_j S,) tensors in place of chunk is that call on the pieces padded to the longest, and
        returns a list of (n_sources, k_j S)"""
        if isinstance(chunk, (list, tuple)):
            return self._call_list(chunk, streams, lengths)
        if streams is None and lengths is not None:
            streams = range(self.num_streams)
        return self._call(chunk, self._select(streams) if streams is not None else None, lengths)

    def flush(self, streams=None):
        """the last L - S samples of every stream (num_streams, n_sources, L - S); then every stream is reset.  With `streams`: of the selected
        streams in the order given, (A, n_sources, L - S), and only they are reset"""
        idx = self._select(streams) if streams is not None else None
        with torch.no_grad():
            out = self.tail.clone() if idx is None else self.tail.index_select(0, torch.tensor(idx, dtype=torch.int64).to(self.device))
        self.reset(idx)
        return out

    def reset(self, streams=None):
        """zero the state of the selected streams (None: all; a list of indices; a bool mask of num_streams); the others are untouched"""
        Bs = self.num_streams
        if streams is None:
            sel = torch.ones(Bs, dtype=torch.uint8)
        elif torch.is_tensor(streams) and streams.dtype == torch.bool:
            if streams.numel() != Bs:
                raise ValueError("the stream mask has {} entries, the separator has {} streams".format(streams.numel(), Bs))
            sel = streams.reshape(-1).cpu().to(torch.uint8)
        else:
            idx = [int(i) for i in (streams.tolist() if torch.is_tensor(streams) else streams)]
            if any(i < 0 or i >= Bs for i in idx):
                raise ValueError("stream index out of range 0 .. {}".format(Bs - 1))
            sel = torch.zeros(Bs, dtype=torch.uint8)
            sel[idx] = 1
        mask = sel.to(self.device)
        keep = self.delay
        with torch.no_grad():
            backend().online_reset(mask, Bs, self.frames, self.carry if keep else None, keep, self.sums, 2 * self.n_norms,
                                   self.rings if self.ring_len else None, self.ring_len, self.tail if keep else None, self.n_src * keep)

    # ------------------------------------------------------------------ state that travels
    def _state_header(self):
        return dict(version=STATE_FORMAT_VERSION, L=self.L, S=self.S, n_sources=self.n_src, n_norms=self.n_norms, ring_len=self.ring_len,
                    separable=not self.dense, config=self.model.get_config(), dtype=str(self.dtype).replace("torch.", ""))

    def _state_args(self, idx):
        """-> the arguments both state entry points share, the slot list uploaded"""
        keep, A = self.delay, len(idx)
        if self._state_slots is None:
            self._state_slots = torch.zeros(self.num_streams, device=self.device, dtype=torch.int32)
        self._state_slots[:A].copy_(torch.tensor(idx, dtype=torch.int32))
        return (self._state_slots, A, self.frames, self.carry if keep else None, keep, self.sums, 2 * self.n_norms,
                self.rings if self.ring_len else None, self.ring_len, self.tail if keep else None, self.n_src * keep)

    def _state_row_bytes(self):
        return backend().online_state_row_bytes(self.delay, 2 * self.n_norms, self.ring_len, self.n_src * self.delay)

    def export_state(self, streams=None):
        """-> OnlineState: row j holds everything slot streams[j] carries from call to call (frame counter, cLN sums, histories, encoder carry,
        overlap-add tail).  `streams` is what sep(chunk, streams=...) accepts (None: all slots in order).  One launch; the separator is not
        changed, and the state does not refer to it afterwards."""
        idx = list(range(self.num_streams)) if streams is None else self._select(streams)
        row_bytes = self._state_row_bytes()
        with torch.no_grad():
            blob = torch.empty(len(idx), row_bytes, device=self.device, dtype=torch.uint8)      # the kernel writes every byte of a row, padding included
            backend().online_state_export(*self._state_args(idx), blob, row_bytes)
        return OnlineState(blob, self._state_header())

    def import_state(self, state, streams=None):
        """Slot streams[j] takes row j of `state` (None: slots 0 .. len(state) - 1, and len(state) must then be num_streams) and goes on exactly as
        the exported slot would have: the same calls give the same bits.  The separator may have any num_streams and need not be the one that
        exported; a state on another device is moved first.  One launch, into the existing state buffers in place: recorded steps stay valid, no
        slot that is not named is written.  A header that does not match this separator's model structure, dtype or format version, a row count
        that does not match the selection, a duplicate or out-of-range slot and a blob of the wrong shape or dtype are ValueErrors raised
        before anything is uploaded or launched.  Whether the model's WEIGHTS are those of the exporting one cannot be checked cheaply and is
        NOT checked: a state imported under other weights continues as a stream that never existed."""
        if not isinstance(state, OnlineState):
            raise ValueError("import_state takes an OnlineState (got {})".format(type(state).__name__))
        own = self._state_header()
        for k in _HEADER_KEYS:
            if state.header[k] != own[k]:
                if k == "version":
                    raise ValueError("the state has format version {}, this separator reads version {}".format(state.header[k], own[k]))
                raise ValueError("the state does not fit this separator: its {} is {!r}, the separator's {!r}".format(k, state.header[k], own[k]))
        blob, row_bytes = state.blob, self._state_row_bytes()
        if blob.dtype != torch.uint8 or blob.dim() != 2 or blob.shape[1] != row_bytes:
            raise ValueError("the state's blob must be a (rows, {}) uint8 tensor (got {} {})".format(row_bytes, tuple(blob.shape), blob.dtype))
        if streams is None:
            if len(state) != self.num_streams:
                raise ValueError("the state has {} rows, the separator {} slots: name the slots that take them".format(len(state), self.num_streams))
            idx = list(range(self.num_streams))
        else:
            idx = self._select(streams)
            if len(idx) != len(state):
                raise ValueError("{} rows of state for {} selected streams: every stream takes one".format(len(state), len(idx)))
        with torch.no_grad():
            blob = blob.to(self.device).contiguous()
            backend().online_state_import(*self._state_args(idx), blob, row_bytes)

    # ------------------------------------------------------------------ a call on a selection of the streams
    def _select(self, streams):
        """-> the selected stream indices in call order, checked: the kernels take the list as it is"""
        Bs = self.num_streams
        if torch.is_tensor(streams) and streams.dtype == torch.bool:
            if streams.numel() != Bs:
                raise ValueError("the stream mask has {} entries, the separator has {} streams".format(streams.numel(), Bs))
            idx = torch.nonzero(streams.reshape(-1)).reshape(-1).tolist()
        else:
            idx = [int(i) for i in (streams.reshape(-1).tolist() if torch.is_tensor(streams) else streams)]
        if not idx:
            raise ValueError("the selection of streams is empty")
        if any(i < 0 or i >= Bs for i in idx):
            raise ValueError("stream index out of range 0 .. {}".format(Bs - 1))
        if len(set(idx)) != len(idx):
            raise ValueError("duplicate stream indices in the selection: every selected stream takes one row of the chunk")
        return idx

    # ------------------------------------------------------------------ a call in which every stream brings its own length
    def _frames_of(self, lengths, A, W):
        """-> frames per row, checked"""
        if torch.is_tensor(lengths):
            if lengths.dtype == torch.bool or lengths.is_floating_point() or lengths.is_complex():
                raise ValueError("lengths must be an integer tensor (got {})".format(lengths.dtype))
            lengths = lengths.reshape(-1).tolist()
        else:
            lengths = list(lengths)
            if any(isinstance(v, bool) or int(v) != v for v in lengths):
                raise ValueError("lengths must be integers (got {})".format(lengths))
            lengths = [int(v) for v in lengths]
        if len(lengths) != A:
            raise ValueError("{} lengths for {} rows of the chunk: every row takes one".format(len(lengths), A))
        for v in lengths:
            if v <= 0 or v % self.S or v > W:
                raise ValueError("a length must be a positive multiple of the stride {} and at most the chunk's {} samples (got {})".format(self.S, W, v))
        return [v // self.S for v in lengths]

    def _call(self, chunk, idx, lengths):
        """every call: on the slots `idx` names, row j slot idx[j] (None: all of them, through the plain entry points); row j brings lengths[j]
        samples (None: the whole chunk; else the ragged entry points)"""
        A = self.num_streams if idx is None else len(idx)
        n = self._check_chunk(chunk, None if idx is None else A)
        W = n * self.S
        offs = ldt = None
        if lengths is not None:
            offs = list(itertools.accumulate(self._frames_of(lengths, A, W), initial=0))
            ldt = _round_up(offs[-1], 128)
        with torch.no_grad():
            ws = self._ws.get(n)
            if ws is None:
                ws = self._ws[n] = _Workspace(self, n)
            v = ws.views(A, ldt)
            v.chunk.copy_(chunk.reshape(A, W))
            if idx is not None:
                ws.slots[:A].copy_(torch.tensor(idx, dtype=torch.int32))
            if offs is not None:
                ws.offs[:A + 1].copy_(torch.tensor(offs, dtype=torch.int32))
            if self.chunk_size is None:
                self.chunk_size = W
            step = (v, n, A, ws.slots if idx is not None else None, ws.offs if offs is not None else None)
            if self.record and W == self.chunk_size:
                flat = self.model.flat_parameters()
                if self._flat is not flat:                                      # model.to() since the recordings: their pointers are stale
                    self._seq, self._flat = None, flat
                    self._sub_seqs.clear()
                key = None if idx is None else A if offs is None else (A, ldt)
                seq = self._seq if key is None else self._sub_seqs.get(key)
                if seq is None:
                    seq = sepkernels.Sequence()
                    with sepkernels.recording(seq):
                        self._step(*step)
                    if key is None:
                        self._seq = seq
                    else:
                        self._sub_seqs[key] = seq
                        while len(self._sub_seqs) > self.max_recordings:       # a recording is a launch list: nothing on the device goes with it
                            self._sub_seqs.popitem(last=False)
                else:
                    if key is not None:
                        self._sub_seqs.move_to_end(key)
                    seq.run()
                    if offs is not None:
                        self.replays[key] += 1
            else:
                self._step(*step)
            return v.out.clone()

    def _call_list(self, pieces, streams, lengths):
        if lengths is not None:
            raise ValueError("a list of pieces carries its own lengths: do not pass `lengths` with it")
        idx = self._select(streams) if streams is not None else list(range(self.num_streams))
        if len(pieces) != len(idx):
            raise ValueError("{} pieces for {} selected streams: every stream takes one".format(len(pieces), len(idx)))
        rows = []
        for x in pieces:
            if not torch.is_tensor(x) or x.dim() not in (1, 2) or (x.dim() == 2 and x.shape[0] != 1) or x.device != self.device or x.dtype != self.dtype:
                raise ValueError("a piece is a (1, k*{}) or (k*{},) tensor on {} in {}".format(self.S, self.S, self.device, self.dtype))
            rows.append(x.reshape(-1))
        sizes = [r.numel() for r in rows]
        if any(v <= 0 or v % self.S for v in sizes):
            raise ValueError("a piece's length must be a positive multiple of the stride {} (got {})".format(self.S, sizes))
        chunk = torch.zeros(len(rows), 1, max(sizes), device=self.device, dtype=self.dtype)
        for j, r in enumerate(rows):
            chunk[j, 0, :sizes[j]] = r
        y = self._call(chunk, idx, sizes)
        return [y[j, :, :sizes[j]] for j in range(len(rows))]

    # ------------------------------------------------------------------ the chunk step
    def _check_chunk(self, chunk, rows=None):
        want = self.num_streams if rows is None else rows
        if not torch.is_tensor(chunk) or chunk.dim() != 3 or chunk.shape[0] != want or chunk.shape[1] != 1:
            what = "a chunk is (num_streams={}".format(want) if rows is None else "a chunk for {} selected streams is ({}".format(want, want)
            raise ValueError("{}, 1, k*{}) (got {})".format(what, self.S, tuple(getattr(chunk, "shape", ()))))
        T = chunk.shape[-1]
        if T == 0 or T % self.S:
            raise ValueError("a chunk's length must be a positive multiple of the stride {} (got {})".format(self.S, T))
        if backend().name == "hip" and not chunk.is_cuda:
            raise RuntimeError("online separation runs on the GPU: the chunk is a {} tensor".format(chunk.device))
        if chunk.device != self.device or chunk.dtype != self.dtype:
            raise ValueError("the chunk must be on {} in {} like the separator's state (got {} {})".format(self.device, self.dtype, chunk.device, chunk.dtype))
        return T // self.S

    def _step(self, ws, n, blocks, slots=None, offs=None):
        """one chunk of n frames of `blocks` streams on the matrices `ws` (_Workspace.views): ~5 launches per TCN layer plus encoder, norm,
        bottleneck, mask, decoder and advance (separable=False: conv1, cLN, online unfold, heads -- 4 or 5).  The pointers pick the form, as in
        csrc/online.hip.  Without `slots`: block j is slot j, the plain entry points.  With `slots` (device int32): block j is slot slots[j],
        the sep_online_*_sel entry points.  With `offs` too (device int32, blocks + 1 entries): block j brings offs[j + 1] - offs[j] <= n
        frames, the sep_online_*_rag entry points, and the products run over all ws.ldt columns"""
        K = backend()
        model, sep = self.model, self.model.separator
        Bs, L, S, N, H, Bn, Sc, n_src = blocks, self.L, self.S, self.N, self.H, self.Bn, self.Sc, self.n_src
        taps = "unfold_fwd" if self.dense else "depthwise_fwd"                    # the kernel that keeps a layer's history
        form, sel = ("", ()) if slots is None else ("_sel", (slots,)) if offs is None else ("_rag", (slots, offs))
        encoder, cln_fwd, depthwise, decoder, advance = (getattr(K, "online_" + k + form)
                                                         for k in ("encoder_fwd", "cln_fwd", taps, "decoder_fwd", "advance"))
        T, ldt = (Bs * n if offs is None else ws.ldt), ws.ldt
        keep = self.delay
        sums, sstride = self.sums.view(-1), 2 * self.n_norms
        amax = None
        if sepkernels.gemm_arith() == sepkernels.ARITH_F16X3 and hasattr(K, "absmax"):
            flat = model.flat_parameters()
            K.absmax(flat, ws.amax, flat.numel())            # the operand bound of the chunk's products (alignment gaps of the buffer hold zeros)
            amax = ws.amax

        def cln(x, y, norm, alpha, i):
            cln_fwd(x, alpha, norm.gamma.reshape(-1), norm.beta.reshape(-1), y, sums[2 * i:], sstride, self.frames, Bs, x.shape[0], n, ldt,
                    norm.eps, *sel)

        def heads(v, out, skip, x_res, x_out, li):
            # x_out = Wo v + bo + x_res, total (+)= Ws v + bs as the training path issues them: the (C, ldt) matrices as one block of all streams
            Wo, bo = (out.weight, out.bias) if out is not None else (None, None)
            b = ws.block
            _fn.heads_launch(b[id(v)], T, Wo, bo, skip.weight, skip.bias, b[id(x_res)], b[id(x_out)], b[id(ws.total)], int(li > 0), amax)

        encoder(ws.chunk, model.encoder.conv1d.weight, self.carry if keep else None, self.carry_next if keep else None, ws.w, Bs, N, L, S,
                n, ldt, model.enc_nonlinear == "relu", *sel)
        cln(ws.w, ws.wn, sep.norm1d, None, 0)
        K.pw_gemm(B=1, M=Bn, K=N, T=T, ldt=ldt, A=sep.bottleneck_conv1d.weight, X=ws.wn, Y=ws.xa, bias=sep.bottleneck_conv1d.bias, a_amax=amax)
        x, x_next = ws.xa, ws.xb
        rings = self.rings.view(-1)
        for li, layer in enumerate(self.layers):
            d, P = layer.dilation, layer.kernel_size
            K.pw_gemm(B=1, M=H, K=Bn, T=T, ldt=ldt, A=layer.bottleneck_conv1d.weight, X=x, Y=ws.ha, bias=layer.bottleneck_conv1d.bias, a_amax=amax)
            if self.dense:
                # one norm, the taps unfolded into rows c P + p (history of (P - 1) d frames per channel in the ring), the two full convolutions as heads
                cln(ws.ha, ws.hb, layer.norm1d, layer.nonlinear1d.weight, 1 + li)
                depthwise(ws.hb, rings[self.ring_offsets[li]:], self.ring_len, ws.cols, Bs, H, n, ldt, P, d, *sel)
                out = layer.output_conv1d if layer.dual_head else None
                heads(ws.cols, out, layer.skip_conv1d, x, x_next, li)
                if out is not None:
                    x, x_next = x_next, x
                continue
            dw = layer.separable_conv1d
            cln(ws.ha, ws.hb, layer.norm1d, layer.nonlinear1d.weight, 1 + 2 * li)
            depthwise(ws.hb, dw.depthwise_conv1d.weight, dw.depthwise_conv1d.bias, rings[self.ring_offsets[li]:], self.ring_len, ws.ha,
                      Bs, H, n, ldt, P, d, *sel)
            cln(ws.ha, ws.hb, dw.norm1d, dw.nonlinear1d.weight, 2 + 2 * li)
            out = dw.output_pointwise_conv1d if dw.dual_head else None
            heads(ws.hb, out, dw.skip_pointwise_conv1d, x, x_next, li)
            if out is not None:
                x, x_next = x_next, x
        M = n_src * N
        K.pw_gemm(B=1, M=M, K=Sc, T=T, ldt=ldt, A=sep.mask_conv1d.weight, X=ws.total, Y=ws.m, bias=sep.mask_conv1d.bias, pro_mode=PRO_PRELU,
                  pro_alpha=sep.prelu.weight, epi_flags=EPI_SIGMOID if model.mask_nonlinear == "sigmoid" else 0, a_amax=amax)
        if model.mask_nonlinear != "sigmoid":
            K.softmax_ch_fwd(ws.m, 1, M, T, ldt)
        decoder(ws.w, ws.m, model.decoder.conv_transpose1d.weight, self.tail if keep else None, self.tail_next if keep else None, ws.out,
                Bs, n_src, N, L, S, n, ldt, *sel)
        advance(self.frames, self.carry if keep else None, self.carry_next if keep else None, keep, self.tail if keep else None,
                self.tail_next if keep else None, n_src * keep, Bs, n, *sel)

    def launches_per_chunk(self):
        """launches of one recorded all-streams chunk step (None before the first recorded one; a subset step issues as many)"""
        return len(self._seq) if self._seq is not None else None
