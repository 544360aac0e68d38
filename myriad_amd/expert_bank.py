"""Bookkeeping of the vision expert's per-class reference bank (vision_expert.py: add_references / one_shot_banked): which
rows of the contiguous per-tap bank tensors belong to which class.  Device-free: the tensors live in VisionExpertHIP, this
class only says where a class's rows are and how the tensors have to be cut when a class leaves."""
from __future__ import annotations

from typing import Dict, List, Tuple


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

    def remove(self, name: str) -> Tuple[int, int]:
        """Forget a class; returns the (offset, rows) it held: the caller cuts those rows out of every tap's tensor and the
        classes behind it move down by `rows`."""
        cut = self.lookup(name)
        del self._rows[name]
        return cut
