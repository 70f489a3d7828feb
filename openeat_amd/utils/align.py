"""Times for CTC alignments (ASRModel.ctc_align).  Pure Python, no device."""
from typing import Tuple


def frame_times(start_frame: int, end_frame: int, subsampling_rate: int, frame_shift_ms: float = 10) -> Tuple[float, float]:
    """Encoder frames [start_frame, end_frame] (inclusive) -> (start_s, end_s) in seconds: an encoder frame covers
    `subsampling_rate` feature frames of `frame_shift_ms` each, and the span ends where frame end_frame + 1 begins."""
    step = subsampling_rate * frame_shift_ms
    return start_frame * step / 1000, (end_frame + 1) * step / 1000
