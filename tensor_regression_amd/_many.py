"""What the many-model entry points of the model modules share: per-model arguments, the argument
prelude, one parameter arena for a whole batch, the result lines and the report.  The engine is reached
as `_engine.<name>` at call time, never bound at import: the host tests replace those functions and
expect every argument error before any of them is touched."""
import itertools

import torch

from . import _engine, _fit


def per_member(name, value, M, one_value=None):
    """One value for all M models, or a list or tuple of M values (ValueError on another length).  Where one
    value is itself a sequence, `one_value(value)` tells the two apart and only a list can be per model."""
    if one_value is None:
        per = isinstance(value, (list, tuple))
    else:
        per = isinstance(value, list) and not one_value(value)
    if not per:
        return [value] * M
    if len(value) != M:
        raise ValueError(f"{name}: a list must hold one value per model ({M}), got {len(value)}")
    return list(value)


def check_models(models, cls, verbose, verbose_2_prints):
    """The argument prelude of a fit_Adam_many: verbose=2 is refused (`verbose_2_prints`: the module's
    own words for what it would print), no model object twice, every model of the module's class."""
    if verbose == 2:
        raise NotImplementedError(f"fit_Adam_many: verbose=2 prints every iteration{verbose_2_prints}; call fit_Adam "
                                  "on each model instead")
    if len({id(m) for m in models}) != len(models):
        raise ValueError("fit_Adam_many: the same model object appears twice")
    for m in models:
        if not isinstance(m, cls):
            raise TypeError(f"fit_Adam_many takes this module's {cls.__name__} objects, got {type(m).__name__}")


def start_report(report, **fields):
    """`report` (a dict or None) emptied and set to the fields of a call that has done nothing yet."""
    if report is not None:
        report.clear()
        report.update(fields)


def pack_members(members_params, device):
    """Every member's parameter tensors in ONE float32 arena on `device` (one launch to pack, one to write
    back): (arena, the offset of every tensor in the order given, a slice of the arena per member)."""
    srcs = [t.detach().reshape(-1) for params in members_params for t in params]
    bounds = [0] + list(itertools.accumulate(s.numel() for s in srcs))
    arena = _engine._pack_arena(srcs, bounds[-1], torch.float32, device)
    last = list(itertools.accumulate(len(params) for params in members_params))
    slices = [arena[bounds[e - len(params)]:bounds[e]] for params, e in zip(members_params, last)]
    return arena, bounds[:-1], slices


def unpack_members(arena, offsets, members_params):
    """pack_members' inverse: the arena's segments copied back into the members' tensors in place."""
    _engine._unpack_arena(arena, offsets, [t for params in members_params for t in params])


def finish_many(results, verbose, report, **report_fields):
    """The end of a many-model call: a line per model for verbose >= 1 (`results`: each model's
    convergence_reached), `report` updated with the call's fields; returns `results`."""
    if (verbose is True) or (verbose >= 1):
        for j, conv in enumerate(results):
            print(f"model {j}: " + _fit.convergence_line(conv))
    if report is not None:
        report.update(report_fields)
    return results
