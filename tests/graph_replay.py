"""Graph replay on a side stream: what production does with every launch, and no kernel test did.

The kernel tests launch on the stream current in the test, which is always the default stream, and read their results
after a device synchronisation.  A launch that ignored its ``stream`` argument, an entry point that copied something
through the host, or one that read a value on the host at call time would pass them all.  StereoNode, ConfidenceNode and
ResizeNode run every launch on a stream of their own and ForwardGraph captures on a side stream, so the property that
matters is: the call is a pure, stream-ordered function of device memory.  ``assert_replays`` checks exactly that by
capturing the call once and replaying it on other data:

1. eager, on the default stream, with values ``a`` and then ``b``: the expected bits (and every code object loaded
   before any capture);
2. capture on a side stream with ``a`` in place and every output spoiled: a capture that raises is a host
   synchronisation, an allocation or a default-stream launch inside the entry point; outputs that changed by the end
   of the capture are a launch that left the captured stream;
3. replay with ``b`` in place: bitwise the eager result for ``b``, so nothing was read on the host at capture time;
4. spoil, put ``a`` back, replay: bitwise the eager result for ``a``, so no call depends on state the last one left.
"""
import ctypes

import torch

SPOIL = 0xA5


def stream():
    """The current torch stream as the ``void* stream`` of the C ABI (inside a capture: the capturing stream)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    assert t.is_contiguous(), "graph_replay: inputs and outputs are whole contiguous tensors"
    return t.view(-1).view(torch.uint8)


def _put(inputs, values) -> None:
    assert len(inputs) == len(values)
    for t, v in zip(inputs, values):
        assert t.shape == v.shape and t.dtype == v.dtype, (t.shape, v.shape, t.dtype, v.dtype)
        t.copy_(v)


def _spoil(outputs) -> None:
    for t in outputs:
        _bytes(t).fill_(SPOIL)


def _spoiled(ts) -> list:
    return [torch.full_like(_bytes(t), SPOIL) for t in ts]


def _differ(got, want) -> list:
    return [i for i, (g, w) in enumerate(zip(got, want)) if not torch.equal(_bytes(g), _bytes(w))]


def _eager(launch, inputs, values, outputs):
    _put(inputs, values)
    _spoil(outputs)
    torch.cuda.synchronize()
    launch()
    torch.cuda.synchronize()
    return [t.clone() for t in outputs]


def assert_replays(launch, inputs, a, b, outputs, what: str = "") -> None:
    """``launch()`` enqueues the call under test on the CURRENT stream (``stream()`` above) and nothing else;
    ``inputs`` are the device tensors it reads, at fixed addresses; ``a`` and ``b`` two sets of values for them (same
    shapes and dtypes, on any device); ``outputs`` every tensor the call writes whose content is a defined result."""
    inputs, outputs = list(inputs), list(outputs)
    assert torch.cuda.current_stream() == torch.cuda.default_stream(), "graph_replay starts on the default stream"
    want_a = _eager(launch, inputs, a, outputs)
    want_b = _eager(launch, inputs, b, outputs)
    assert _differ(want_a, want_b), f"{what}: the two sets of values give the same outputs: a replay would show nothing"
    unwritten = [i for i in range(len(outputs)) if i not in _differ(want_a, _spoiled(want_a))]
    assert not unwritten, f"{what}: outputs {unwritten} are not written by the call"

    _put(inputs, a)
    _spoil(outputs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    captured = False
    try:
        try:
            with torch.cuda.graph(graph, stream=side):
                launch()
            captured = True
        except Exception as e:  # noqa: BLE001  (whatever the runtime or the library raises: the message is the finding)
            raise AssertionError(f"{what}: the call cannot be captured on a side stream (a host synchronisation, an "
                                 f"allocation or a default-stream launch inside it): {type(e).__name__}: {e}") from e
        torch.cuda.synchronize()
        ran = _differ(outputs, _spoiled(outputs))
        assert not ran, (f"{what}: outputs {ran} were written while the call was being captured: a launch left the "
                         "captured stream")

        for tag, values, want in (("new data", b, want_b), ("the first data again", a, want_a)):
            _spoil(outputs)
            _put(inputs, values)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                graph.replay()
            torch.cuda.synchronize()
            bad = _differ(outputs, want)
            assert not bad, (f"{what}: replay on {tag}: outputs {bad} differ from the eager call on the same values "
                             "(a value read on the host at capture time, a launch outside the graph, or state kept "
                             "between calls)")
    finally:
        if captured:
            graph.reset()  # one graph alive at a time
        del graph
