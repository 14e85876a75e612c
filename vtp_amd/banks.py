"""What ZeroShot, ReconEval, LinearProbe, Knn, PrecisionRecall, Retrieval and KID share around their kernels, written once: the
device, the process group, growable banks of feature rows and their rank-major gather, the pass-over-chunks loop, the grow-only
workspace and the check of a batch of feature rows.  Plain torch: but for the device checks it works on CPU tensors as well."""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch


def eval_device(owner: str, model=None, device=None) -> torch.device:
    """the device of an evaluation class: `device`, else the model's, else the current GPU; anything but a GPU raises"""
    if not torch.cuda.is_available():
        raise RuntimeError(f"vtp_amd.{owner} runs on the MI355X kernels only (no CPU fallback)")
    if device is None:
        device = next(model.parameters()).device if model is not None else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"vtp_amd.{owner} runs on the MI355X kernels only: the model / device must be cuda (no CPU fallback)")
    return device


class Group:
    """a process group (None: this process alone); torch.distributed is imported only when one is given"""

    def __init__(self, group=None):
        self.group, self.world, self.rank = group, 1, 0
        if group is not None:
            import torch.distributed as dist
            self.dist = dist
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)

    def summed(self, t: torch.Tensor) -> torch.Tensor:
        """t summed over the group with one all-reduce (a copy; t itself without a group)"""
        if self.world > 1:
            t = t.clone()
            self.dist.all_reduce(t, group=self.group)
        return t

    def all_gather(self, t: torch.Tensor) -> List[torch.Tensor]:
        """t of every rank, in rank order (the gloo backend gathers host tensors only: staged through the host there)"""
        host = self.dist.get_backend(self.group) == "gloo"
        src = t.cpu() if host else t
        parts = [torch.empty_like(src) for _ in range(self.world)]
        self.dist.all_gather(parts, src, group=self.group)
        return [p.to(t.device) for p in parts] if host else parts

    def all_gather_rows(self, out: torch.Tensor, inp: torch.Tensor) -> None:
        """out [world * B, ...] = the rows inp [B, ...] of every rank in rank order: RCCL all-gather into the tensor, or zero + copy +
        all_reduce on backends without it"""
        if self.dist.get_backend(self.group) == "nccl":
            self.dist.all_gather_into_tensor(out, inp, group=self.group)
        else:
            B = inp.shape[0]
            out.zero_()
            out[self.rank * B:(self.rank + 1) * B].copy_(inp)
            self.dist.all_reduce(out, group=self.group)


def spans(n: int, step: int) -> Iterator[Tuple[int, int]]:
    """(lo, hi) of the pieces of at most `step` that cover range(n), in order"""
    for lo in range(0, n, step):
        yield lo, min(n, lo + step)


class Workspace:
    """a grow-only uint8 buffer"""

    def __init__(self, device):
        self.buf = torch.empty(0, device=device, dtype=torch.uint8)

    def at_least(self, need: int) -> torch.Tensor:
        if self.buf.numel() < need:
            self.buf = torch.empty(need, device=self.buf.device, dtype=torch.uint8)
        return self.buf


def aligned_f32(t: torch.Tensor) -> torch.Tensor:
    """t detached and as f32, copied only where the kernels' 16-byte row alignment asks for it"""
    f = t.detach().to(torch.float32)
    if f.stride(1) != 1 or f.stride(0) % 4 or f.data_ptr() % 16:
        f = f.contiguous()
    return f


def feature_rows(feats: torch.Tensor, what: str, width: Optional[int] = None, align: bool = False) -> torch.Tensor:
    """a batch of feature rows as the evaluations take it: on the device, [n >= 1, D] with D a positive multiple of 8 (and `width`,
    where the bank has one); returned detached and as f32, with align=True laid out for a kernel that reads it directly"""
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise ValueError(f"{what} must live on the MI355X (got a CPU tensor): there is no CPU path")
    if feats.dim() != 2 or feats.shape[0] < 1 or feats.shape[1] < 8 or feats.shape[1] % 8:
        raise ValueError(f"{what} must be [n, D] with n >= 1 and D a multiple of 8, got {tuple(feats.shape)}")
    if width is not None and feats.shape[1] != width:
        raise ValueError(f"{what} must be [n, {width}] like the bank, got {tuple(feats.shape)}")
    return aligned_f32(feats) if align else feats.detach().to(torch.float32)


class Bank:
    """growable rows f32 [capacity, D] with the integer columns {name: dtype} beside them; `capacity` rows at first, doubled when full"""

    def __init__(self, device, capacity: Optional[int] = None, columns: Optional[Dict[str, torch.dtype]] = None):
        self._capacity0, self.dtypes = capacity, dict(columns or {})
        self._rows = torch.empty(0, 0, device=device, dtype=torch.float32)
        self._columns = {c: torch.empty(0, device=device, dtype=dt) for c, dt in self.dtypes.items()}
        self.size = 0  # rows in use

    capacity = property(lambda self: self._rows.shape[0], doc="rows allocated")
    width = property(lambda self: self._rows.shape[1] if self.size else None, doc="D of the rows in use; None without any")

    def reserve(self, n: int, D: int) -> Tuple[torch.Tensor, ...]:
        """makes room for n more rows of width D and returns the views to fill: (rows [n, D], then one [n] per column)"""
        size = self.size
        if size and D != self.width:
            raise ValueError(f"rows must be [n, {self.width}] like the bank, got [{n}, {D}]")
        if self._rows.shape[1] != D or size + n > self.capacity:
            cap = self.capacity or max(self._capacity0 or 0, 1)
            while cap < size + n:
                cap *= 2
            old = (self._rows, *self._columns.values())
            self._rows = torch.empty(cap, D, device=self._rows.device, dtype=torch.float32)
            self._columns = {c: torch.empty(cap, device=self._rows.device, dtype=dt) for c, dt in self.dtypes.items()}
            if size:
                for new, t in zip((self._rows, *self._columns.values()), old):
                    new[:size].copy_(t[:size])
        self.size = size + n
        return tuple(t[size:size + n] for t in (self._rows, *self._columns.values()))

    @property
    def rows(self) -> torch.Tensor:
        """the rows in use, f32 [size, D] (a view)"""
        return self._rows[:self.size]

    def column(self, name: str) -> torch.Tensor:
        """the entries in use of a column, [size] (a view)"""
        return self._columns[name][:self.size]

    def clear(self) -> None:
        """forgets the rows and keeps the storage"""
        self.size = 0


class BankSet:
    """named banks of one width (the real and the generated rows, the image and the text rows) and their gather over a group"""

    def __init__(self, names: Sequence[str], device, capacity: Optional[int] = None, columns: Optional[Dict[str, torch.dtype]] = None):
        self.device = device
        self.banks = {name: Bank(device, capacity, columns) for name in names}

    def __getitem__(self, name: str) -> Bank:
        return self.banks[name]

    def check_width(self, shape, what: str) -> None:
        for name, bank in self.banks.items():
            if bank.width is not None and bank.width != shape[1]:
                raise ValueError(f"{what} must be [n, {bank.width}] like the {name} bank, got {tuple(shape)}")

    def append(self, name: str, feats: torch.Tensor, what: str) -> None:
        """the rows of feats [n, D] (feature_rows) at the end of one bank"""
        f = feature_rows(feats, what)
        self.check_width(f.shape, what)
        self.banks[name].reserve(*f.shape)[0].copy_(f)

    def clear(self) -> None:
        for bank in self.banks.values():
            bank.clear()

    def gathered(self, group: Group) -> Tuple[Dict[str, torch.Tensor], Dict[str, Dict[str, torch.Tensor]], Dict[str, int]]:
        """(rows {bank: f32 [N, D]}, columns {bank: {column: [N]}}, totals {bank: N}) of the whole group, rank-major (this rank's views
        without one): the counts and the width are exchanged, then each shard is padded to the largest, gathered and cut.  Without
        a width on any rank nothing is gathered; zero totals, of the set or of one bank, are the caller's to refuse."""
        if group.world == 1:
            return ({s: b.rows for s, b in self.banks.items()}, {s: {c: b.column(c) for c in b.dtypes} for s, b in self.banks.items()},
                    {s: b.size for s, b in self.banks.items()})
        D = next((b.width for b in self.banks.values() if b.width is not None), 0)
        mine = torch.tensor([b.size for b in self.banks.values()] + [D], device=self.device, dtype=torch.int64)
        every = torch.stack(group.all_gather(mine)).cpu()
        widths = {int(d) for d in every[:, -1] if int(d)}
        if len(widths) > 1:
            raise ValueError(f"the ranks hold features of different widths: {sorted(widths)}")
        rows, columns, totals = {}, {}, {s: int(every[:, c].sum()) for c, s in enumerate(self.banks)}
        if not widths:
            return rows, columns, totals
        D = widths.pop()
        for c, (s, bank) in enumerate(self.banks.items()):
            sizes = [int(n) for n in every[:, c]]

            def whole(mine: torch.Tensor, *tail: int) -> torch.Tensor:
                shard = torch.zeros(max(max(sizes), 1), *tail, device=self.device, dtype=mine.dtype)
                if bank.size:
                    shard[:bank.size].copy_(mine)
                return torch.cat([p[:n] for p, n in zip(group.all_gather(shard), sizes)])

            rows[s] = whole(bank.rows, D)
            columns[s] = {name: whole(bank.column(name)) for name in bank.dtypes}
        return rows, columns, totals
