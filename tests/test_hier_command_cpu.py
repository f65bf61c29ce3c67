"""What the hierarchy commands share (hgs._hier_command) without a GPU: the option walk, the side-file helpers on a
directory of their own, the tail carry on hand-made tensors, the exits.  The commands' own parsers and round trips are in
the tests of each tool."""
import torch

from hgs import _hier_command as hc
from hgs.hierarchy import Hierarchy

ARITY = {"--leaf": 1, "--half": 0, "--roi": 6, "--view": 3}


def test_the_walker_takes_options_wherever_they_stand():
    pos, seen = hc.walk_args(["--leaf", "keep", "a.hier", "--half", "b.hier", "--view", "0", "-2", "-1e-3"], ARITY)
    assert pos == ["a.hier", "b.hier"]
    assert seen == {"--leaf": [["keep"]], "--half": [[]], "--roi": [], "--view": [["0", "-2", "-1e-3"]]}
    # negative numbers are values, and positionals even outside an option's window
    assert hc.walk_args(["-2", "--half", "-1e-3"], ARITY) == (["-2", "-1e-3"], dict(seen, **{"--leaf": [], "--view": []}))
    # two occurrences in order, an absent option []
    pos, seen = hc.walk_args(["a", "--view", "1", "2", "3", "b", "--view", "4", "5", "6", "--half", "--half"], ARITY)
    assert pos == ["a", "b"] and seen["--view"] == [["1", "2", "3"], ["4", "5", "6"]] and seen["--half"] == [[], []]
    assert seen["--leaf"] == [] and seen["--roi"] == []
    assert hc.walk_args([], ARITY) == ([], {k: [] for k in ARITY})


def test_the_walker_refuses_unknown_options_and_short_windows():
    assert hc.walk_args(["a", "b", "--frobnicate"], ARITY) is None
    assert hc.walk_args(["a", "b", "--leaf"], ARITY) is None                            # the last token
    assert hc.walk_args(["a", "b", "--roi", "0", "0", "0", "1", "1"], ARITY) is None    # n - 1 tokens left
    assert hc.walk_args(["--view", "0", "0"], ARITY) is None
    # a --name inside an option's window is that option's value, known or not: the caller's conversion refuses it
    pos, seen = hc.walk_args(["a", "--roi", "0", "0", "0", "1", "1", "--half", "b", "--view", "--x", "--leaf", "1"], ARITY)
    assert pos == ["a", "b"] and seen["--roi"] == [["0", "0", "0", "1", "1", "--half"]] and seen["--half"] == []
    assert seen["--view"] == [["--x", "--leaf", "1"]] and seen["--leaf"] == []
    # the argument list is left as it was, and the occurrences are lists of their own
    argv = ["a", "--leaf", "cube"]
    hc.walk_args(argv, ARITY)[1]["--leaf"][0].append("x")
    assert argv == ["a", "--leaf", "cube"]


def test_the_side_file_helpers(tmp_path):
    src, other = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    other.mkdir()
    (src / "anchors.bin").write_bytes(b"\x01\x02\x03")
    in_path = str(src / "a.hier")
    assert hc.SIDE_FILES == ("anchors.bin", "exposure.json")
    assert hc.side_files_beside(in_path) == ["anchors.bin"]
    assert hc.carry_side_files(in_path, str(other / "b.hier")) == (["anchors.bin"], False)
    assert (other / "anchors.bin").read_bytes() == b"\x01\x02\x03" and not (other / "exposure.json").exists()
    assert sorted(p.name for p in other.iterdir()) == ["anchors.bin"]
    assert hc.carry_side_files(in_path, str(src / "b.hier")) == (["anchors.bin"], True)
    assert sorted(p.name for p in src.iterdir()) == ["anchors.bin"] and (src / "anchors.bin").read_bytes() == b"\x01\x02\x03"
    assert hc.side_files_beside(str(other / "b.hier")) == ["anchors.bin"] and hc.side_files_beside(str(tmp_path / "x")) == []


def _hier(G, N, base):
    g = torch.Generator().manual_seed(base)
    r = lambda *s: torch.rand(*s, generator=g) + base
    return Hierarchy(r(G, 3), r(G, 16, 3), r(G, 1), r(G, 3), r(G, 4), torch.zeros(N, 7, dtype=torch.int32), r(N, 2, 4))


def test_with_tail_carries_the_rows_behind_the_nodes():
    bits = lambda t: t.contiguous().view(torch.int32)
    for N, G in ((3, 5), (3, 3)):
        host, kept = _hier(G, N, 1), _hier(2, 2, 7)            # two of the N node rows kept on the "device"
        rows = hc.with_tail(kept, host, N)
        assert len(rows) == len(hc.ROWS) == 5
        for k, t in zip(hc.ROWS, rows):
            assert t.shape == (2 + G - N,) + getattr(host, k).shape[1:] and t.dtype == torch.float32, k
            assert torch.equal(bits(t[:2]), bits(getattr(kept, k))), k
            assert torch.equal(bits(t[2:]), bits(getattr(host, k)[N:])), k
    assert hc.NAMES == hc.ROWS + ("nodes", "boxes")


def test_the_exits(tmp_path, capsys):
    assert hc.usage_exit("usage: tool <in>") == 2
    assert capsys.readouterr() == ("", "usage: tool <in>\n")
    assert hc.usage_exit("usage: tool <in>", "tool: refused") == 2
    assert capsys.readouterr() == ("", "tool: refused\nusage: tool <in>\n")
    here = tmp_path / "here.hier"
    here.write_bytes(b"")
    assert hc.missing_path("tool", str(here), None) is False
    assert capsys.readouterr() == ("", "")
    gone, gone2 = str(tmp_path / "gone.hier"), str(tmp_path / "gone.json")
    assert hc.missing_path("tool", str(here), None, gone, gone2) is True
    assert capsys.readouterr() == ("", f"tool: {gone} does not exist\n")
    assert hc.check_exit("tool", "in.hier: acyclic (node 3): a cycle") == 1
    assert capsys.readouterr() == ("", "tool: in.hier: acyclic (node 3): a cycle; nothing written\n")
