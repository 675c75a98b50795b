"""What combines of early termination and occupancy gating, over every combination of t_stop, t_stop_count, occupancy,
occupancy_count and autograd, through a VolumeRenderer call and through GraphedRenderer.__init__, against a literal
table recorded from the code before avr.renderers.check_skip_modes existed (one statement of rules that were
written out four times). No device: the net is the torch.nn.Identity stub of the other CPU tests, so a call the mode
rules accept goes on to the next refusal -- the net is not on the fused path, or the first launch finds no device --
and that counts as accepted here; GraphedRenderer's capture is stubbed out, its __init__ checks run."""
import itertools

import pytest
import torch

T_STOP = (None, 1e-3)
COUNT = ("host", "device")
OCC = (False, True)
GRAD = (False, True)
VIA = ("renderer", "graphed")

# "-": accepted; "m": refused by the mode rules (ValueError); "g": refused because a grid needs torch.no_grad()
# (ValueError). Row: (t_stop, t_stop_count, occupancy set, occupancy_count); columns: renderer without / with autograd,
# GraphedRenderer without / with autograd.
TABLE = {
    (None, 'host', False, 'host'): "----",
    (None, 'host', False, 'device'): "----",
    (None, 'host', True, 'host'): "-gmm",
    (None, 'host', True, 'device'): "-g--",
    (None, 'device', False, 'host'): "----",
    (None, 'device', False, 'device'): "----",
    (None, 'device', True, 'host'): "-gmm",
    (None, 'device', True, 'device'): "-g--",
    (0.001, 'host', False, 'host'): "--mm",
    (0.001, 'host', False, 'device'): "--mm",
    (0.001, 'host', True, 'host'): "mgmm",
    (0.001, 'host', True, 'device'): "mgmm",
    (0.001, 'device', False, 'host'): "----",
    (0.001, 'device', False, 'device'): "----",
    (0.001, 'device', True, 'host'): "-gmm",
    (0.001, 'device', True, 'device'): "-g--",
}


def _grid():
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid.all_occupied((-1, -1, -1), (1, 1, 1), (32, 32, 32), "cpu")


def outcome(t_stop, t_stop_count, occ, occupancy_count, grad, via):
    from avr._lib import AVRError
    from avr.graphs import GraphedRenderer
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.t_stop, rend.t_stop_count = t_stop, t_stop_count
    rend.occupancy, rend.occupancy_count = _grid() if occ else None, occupancy_count
    R = 8
    args = (torch.eye(4).reshape(1, 1, 4, 4).expand(1, R, 4, 4), torch.eye(3)[None], torch.rand(1, R, 2))
    try:
        with torch.set_grad_enabled(grad):
            if via == "graphed":
                GraphedRenderer(rend, torch.nn.Identity(), *args)
            else:
                rend(*args, torch.nn.Identity())
    except AVRError as e:
        assert "no CPU path" in str(e)
    except ValueError as e:
        if "no_grad" in str(e):
            return "g"
        if "fused path" not in str(e):
            return "m"
    return "-"


def test_every_combination_is_accepted_or_refused_as_before(monkeypatch):
    from avr.graphs import GraphedRenderer
    monkeypatch.setattr(GraphedRenderer, "_capture", lambda self: None)
    rows = list(itertools.product(T_STOP, COUNT, OCC, COUNT))
    assert sorted(TABLE, key=repr) == sorted(rows, key=repr)
    got = {row: "".join(outcome(*row, grad, via) for via in VIA for grad in GRAD) for row in rows}
    assert got == TABLE
