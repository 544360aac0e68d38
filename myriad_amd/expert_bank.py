"""Bookkeeping of the vision expert's per-class reference bank (vision_expert.py: add_references / one_shot_banked): which
rows of the contiguous per-tap bank tensors belong to which class.  Device-free: the tensors live in VisionExpertHIP, this
class only says where a class's rows are and how the tensors have to be cut when a class leaves or shrinks to a coreset."""
from __future__ import annotations

import math
import numbers
from typing import Dict, List, Tuple


def keep_rows(keep, rows: int) -> int:
    """How many of a class's `rows` bank rows a coreset keeps (compact_references): an int is the row count itself, 1..rows; a
    float in (0, 1] is the share, max(1, ceil(keep * rows)).  ValueError for anything else (1 is one row, 1.0 is every row)."""
    if isinstance(keep, bool) or not isinstance(keep, (numbers.Integral, float)):
        raise ValueError(f"keep must be an int row count or a float share in (0, 1], got {keep!r}")
    if isinstance(keep, numbers.Integral):
        if not 1 <= int(keep) <= rows:
            raise ValueError(f"keep = {keep} rows is outside 1..{rows}")
        return int(keep)
    if not 0.0 < keep <= 1.0:
        raise ValueError(f"keep = {keep} is not a share in (0, 1]")
    return min(rows, max(1, math.ceil(keep * rows)))


class BankIndex:
    """Classes in the order they were added, each a run of `rows` consecutive bank rows; the runs are contiguous from row 0
    with no gaps, so a class's offset is the row count of the classes before it."""

    def __init__(self):
        self._rows: Dict[str, int] = {}                    # insertion-ordered

    def __contains__(self, name: str) -> bool:
        return name in self._rows

    def __len__(self) -> int:
        return len(self._rows)

    def names(self) -> List[str]:
        return list(self._rows)

    @property
    def total(self) -> int:
        return sum(self._rows.values())

    def lookup(self, name: str) -> Tuple[int, int]:
        """(offset, rows) of a registered class; KeyError naming the class otherwise."""
        if name not in self._rows:
            raise KeyError(f"reference bank has no class {name!r} (registered: {self.names()}); add_references() it first")
        off = 0
        for n, r in self._rows.items():
            if n == name:
                return off, r
            off += r
        raise AssertionError("unreachable")

    def append(self, name: str, rows: int) -> int:
        """Register a new class of `rows` rows behind the last one; returns its offset (the bank's row count so far)."""
        if name in self._rows:
            raise ValueError(f"class {name!r} is registered: remove() it before appending its replacement")
        if int(rows) < 1:
            raise ValueError(f"class {name!r}: a class needs at least one bank row, got {rows}")
        off = self.total
        self._rows[name] = int(rows)
        return off

    def resize(self, name: str, rows: int) -> Tuple[int, int]:
        """A class keeps `rows` of its rows (compact_references); returns the (offset, rows) it held: the caller replaces
        those rows of every tap's tensor by the `rows` kept ones and the classes behind it move down by the difference.  The
        class keeps its place in the order."""
        off, old = self.lookup(name)
        if not 1 <= int(rows) <= old:
            raise ValueError(f"class {name!r} holds {old} bank rows: cannot resize it to {rows} (1..{old})")
        self._rows[name] = int(rows)
        return off, old

    def remove(self, name: str) -> Tuple[int, int]:
        """Forget a class; returns the (offset, rows) it held: the caller cuts those rows out of every tap's tensor and the
        classes behind it move down by `rows`."""
        cut = self.lookup(name)
        del self._rows[name]
        return cut
