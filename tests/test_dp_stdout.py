"""dp.whole_lines: the ranks of a data-parallel job share one stdout, and every test that reads a job's output matches whole
lines (`rank <r> stats <json>`).  An unbuffered interpreter (PYTHONUNBUFFERED=1, `python -u`) writes each print() argument
separately, so two ranks printing at once splice their lines.  No GPU, no processes: the raw stream below records every
write that would reach the shared file."""
import io

from spatial_vae_amd import dp


class _Raw(io.RawIOBase):
    def __init__(self):
        self.writes = []

    def writable(self):
        return True

    def write(self, b):
        self.writes.append(bytes(b))
        return len(b)


def _unbuffered():
    raw = _Raw()
    return raw, io.TextIOWrapper(raw, write_through=True)            # what sys.stdout is under `python -u`


def test_an_unbuffered_stream_splits_a_printed_line():
    """The premise: without whole_lines one print() is several writes."""
    raw, out = _unbuffered()
    print("rank", 0, "stats", "{}", file=out)
    assert len(raw.writes) > 1 and b"".join(raw.writes) == b"rank 0 stats {}\n"


def test_whole_lines_writes_each_line_once_and_at_once():
    raw, out = _unbuffered()
    dp.whole_lines(out)
    print("rank", 0, "stats", "{}", file=out)
    assert raw.writes == [b"rank 0 stats {}\n"]                      # one write, and already out: nothing waits for a flush
    print("a", end="", file=out)
    assert len(raw.writes) == 1
    print("b", 2, file=out)
    assert raw.writes[1:] == [b"ab 2\n"]


def test_whole_lines_leaves_other_streams_alone():
    s = io.StringIO()
    dp.whole_lines(s)
    print("x", 1, file=s)
    assert s.getvalue() == "x 1\n"
