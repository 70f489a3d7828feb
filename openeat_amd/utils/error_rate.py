"""Token error rate from the counts `ops.edit_distance` leaves on the device (the reference scores decodes on the host with
tools/compute-wer.py; the semantics and the tie order are restated in include/openeat_hip.h).  Nothing here reads the device
until `ErrorRate.result()`."""
import torch


class ErrorRate:
    """Running totals of (cor, sub, del, ins) over batches of pairs."""

    def __init__(self):
        self._acc = None                                           # (4) int64 on the device of the first update

    def update(self, counts: torch.Tensor):
        """counts (P, 4) int32 = cor, sub, del, ins per pair; rows of -1 (a slot that does not exist) are skipped.  No sync."""
        c = counts.reshape(-1, 4).to(torch.int64)
        s = (c * (c[:, :1] >= 0)).sum(0)
        self._acc = s if self._acc is None else self._acc + s
        return self

    def result(self) -> dict:
        """The one device-to-host read: all (= cor + sub + del, the reference tokens), cor, sub, del, ins, rate (nan when all == 0)."""
        cor, sub, dele, ins = (0, 0, 0, 0) if self._acc is None else self._acc.tolist()
        n = cor + sub + dele
        return {"all": n, "cor": cor, "sub": sub, "del": dele, "ins": ins, "rate": (sub + dele + ins) / n if n else float("nan")}

    def __str__(self) -> str:
        return overall_line(self.result())


def overall_line(r: dict) -> str:
    """compute-wer.py's overall line for a result() dict (the tool prints 0.00 for an empty reference)."""
    wer = float(r["ins"] + r["sub"] + r["del"]) * 100.0 / r["all"] if r["all"] != 0 else 0.0
    return "Overall -> %4.2f %% " % wer + "N=%d C=%d S=%d D=%d I=%d" % (r["all"], r["cor"], r["sub"], r["del"], r["ins"])


def nbest_oracle(counts: torch.Tensor, beam: int):
    """counts (B * beam, 4) of n-best lists scored against their utterances (ops.edit_distance with group = beam) ->
    (counts_best (B, 4), index (B) int64): per utterance the existing slot with the fewest errors sub + del + ins, the lowest
    index among equals; an utterance without any slot gives index 0 and its row of -1.  On the device, no sync."""
    c = counts.reshape(-1, beam, 4).to(torch.int64)
    err = c[..., 1] + c[..., 2] + c[..., 3]
    err = torch.where(c[..., 0] >= 0, err, torch.full_like(err, 1 << 40))
    key = err * beam + torch.arange(beam, device=c.device)         # unique per utterance: the minimum is the lowest index among equals
    index = key.argmin(1)
    best = counts.reshape(-1, beam, 4).gather(1, index.view(-1, 1, 1).expand(-1, 1, 4)).squeeze(1)
    return best, index
