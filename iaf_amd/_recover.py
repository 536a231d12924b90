"""What TrainStep and EvalPass share around an object that switches kernels (include/iaf_hip.h: IAF_ERR_RANGE, IAF_ERR_EXCHANGE): which
objects of a model keep a range word, which of them raised it since the last look, the compute-only passes that move them, and the
capture of hipGraphs behind those passes."""
import warnings

import torch

from . import _capi

# the errors an object reports once, at its next eager call, about an EARLIER launch whose outputs carry inf / NaN; the object has
# switched kernels and the call can be repeated
SWITCHED = (_capi.RangeError, _capi.ExchangeError)


def range_objects(model):
    """the stacks and convs of a CVAE1 that keep a range word (an object without `layers` has none)"""
    out = []
    for level in getattr(model, "layers", []):
        for layer in level:
            out.append(layer.posterior.stack)
            out.extend(layer.convs())
    return out


def flagged(objects):
    """the indices of the objects whose range word is set"""
    return {i for i, o in enumerate(objects) if o.range_errors()}


def newly_flagged(objects, seen):
    """the indices of the objects whose range word is set and that `seen` does not hold yet; they join `seen`"""
    now = flagged(objects)
    new = now - seen
    seen |= now
    return new


def settle(compute, n_objects, who, on_device=True):
    """Compute-only eager passes (`compute()`: no collective, no update, nothing advances) until two in a row report nothing: each
    report moves one object to bf16 planes (existing protocol), and a pass on the new kernels can overflow further down, which the
    pass after it reports.  Also the warm-up that precedes every capture."""
    clean, limit = 0, 2 * n_objects + 4
    for _ in range(limit):
        if on_device:
            torch.cuda.synchronize()
        try:
            compute()
            clean += 1
        except SWITCHED:
            clean = 0
        if clean == 2:
            if on_device:
                torch.cuda.synchronize()
            return
    raise _capi.IafHipError("%s: objects kept reporting range / exchange failures after %d passes" % (who, limit))


def capture(owner, side, settle_fn, bodies, who, what, stacklevel):
    """One hipGraph per body, in order, on the stream `side`, each attempt behind settle_fn() (the warm-up: workspaces, exchange sets
    and launch caches exist before the capture).  Returns (graphs, what the bodies returned); None after the runtime refused the
    capture -- owner.graph_refused then says why, behind a RuntimeWarning ("<who>: the runtime refused to capture <what> ...")."""
    done = None
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for attempt in range(2):
            settle_fn()
            graphs, results = [torch.cuda.CUDAGraph() for _ in bodies], []
            try:
                for g, body in zip(graphs, bodies):
                    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                        results.append(body())
            except SWITCHED:
                torch.cuda.synchronize()
                continue
            except Exception as e:       # noqa: BLE001
                owner.graph_refused = (str(e).splitlines() or [""])[0]
                warnings.warn("%s: the runtime refused to capture %s (%s): eager launches" % (who, what, owner.graph_refused),
                              RuntimeWarning, stacklevel=stacklevel)
                torch.cuda.synchronize()
                break
            done = (graphs, results)
            break
    torch.cuda.current_stream().wait_stream(side)
    if done is None and owner.graph_refused is None:
        raise _capi.IafHipError("%s: the capture kept meeting objects that switch kernels" % who)
    return done
