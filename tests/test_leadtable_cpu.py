"""The refusals that the four per-lead verification tables share (``_leadtable.py``), no GPU: every row is (class, bad
argument) with the FULL message, compared with ``==`` - the messages are the tables' interface to a log reader, and each
class keeps its own name and noun in them.  The strings were recorded by running these very calls at the commit before
``_leadtable.py`` existed.  The refusals of ``Forecaster.run`` that go over the tables passed follow."""
import numpy as np
import pytest
import torch

from paradis_model_amd.events import EventTable
from paradis_model_amd.neighbourhood import FractionsTable
from paradis_model_amd.spectrum import Spectra
from paradis_model_amd.verify import Scorecard

NAMES = ["tp", "u10", "v10", "t2m"]
H, W = 5, 8
LAT = np.linspace(-80.0, 80.0, H)
EV = {"rain": {"source": "tp", "thresholds": [1.0]}}
GOOD = {
    "Scorecard": (Scorecard, dict(names=NAMES, lat_weights=np.cos(np.deg2rad(LAT)), n_leads=2, device="cpu")),
    "Spectra": (Spectra, dict(names=NAMES, lat_deg=LAT, n_leads=2, device="cpu")),
    "EventTable": (EventTable, dict(names=NAMES, lat_deg=LAT, n_leads=2, events=EV, device="cpu")),
    "FractionsTable": (FractionsTable, dict(names=NAMES, lat_deg=LAT, n_lon=W, n_leads=2, events=EV, scales=[0, 1],
                                            device="cpu")),
}
WEIGHTS = {"Scorecard": "lat_weights", "Spectra": "weights", "EventTable": "weights", "FractionsTable": "weights"}
X = torch.zeros(2, 4, H, W)
K32 = torch.zeros(2, dtype=torch.int32)
CLIM1, CLIM2 = torch.zeros(1, 4, H, W), torch.zeros(2, 4, H, W)


def new(who, **kw):
    cls, good = GOOD[who]
    if "weights" in kw:
        kw[WEIGHTS[who]] = kw.pop("weights")
    return cls(**{**good, **kw})


def update(who, *args, **kw):
    """``update`` of a good table made with ``kw``; Spectra.update takes no clim_index"""
    return new(who, **kw).update(*args)


# (class, bad argument, the call, the full message)
ALL, LATS, CLIMS = tuple(GOOD), ("Spectra", "EventTable", "FractionsTable"), ("Scorecard", "EventTable", "FractionsTable")
CONSTRUCTOR = {
    "names=[]": (ALL, lambda who: new(who, names=[])),
    "n_leads=0": (ALL, lambda who: new(who, n_leads=0)),
    "n_leads=True": (ALL, lambda who: new(who, n_leads=True)),
    "a latitude of 91": (LATS, lambda who: new(who, lat_deg=[0.0, 91.0, 10.0, 20.0, 30.0])),
    "weights of the wrong length": (LATS, lambda who: new(who, weights=torch.ones(H + 1))),
    "integer weights": (ALL, lambda who: new(who, weights=torch.ones(H, dtype=torch.int64))),
    "negative weights": (ALL, lambda who: new(who, weights=-torch.ones(H))),
    "bands={}": (LATS, lambda who: new(who, bands={})),
    "a band that holds no row": (LATS, lambda who: new(who, bands={"x": (81, 90)})),
    "a band with lo > hi": (LATS, lambda who: new(who, bands={"x": (10, -10)})),
    "a band that is no pair": (LATS, lambda who: new(who, bands={"x": 3})),
    "a float64 climatology": (CLIMS, lambda who: new(who, climatology=CLIM2.double())),
    "a climatology of 3 channels": (CLIMS, lambda who: new(who, climatology=torch.zeros(2, 3, H, W))),
    "n_lon=0": (("FractionsTable",), lambda who: new(who, n_lon=0)),
}
UPDATE = {
    "lead=True": (ALL, lambda who: update(who, True, X, X)),
    "lead=2": (ALL, lambda who: update(who, 2, X, X)),
    "a 3-d forecast": (ALL, lambda who: update(who, 0, X[0], X)),
    "a float64 truth": (ALL, lambda who: update(who, 0, X, X.double())),
    "3 channels": (ALL, lambda who: update(who, 0, X[:, :3], X[:, :3])),
    "a truth of another shape": (ALL, lambda who: update(who, 0, X, X[:1])),
    "a state that is not dense": (ALL, lambda who: update(who, 0, torch.zeros(2, 4, H, 2 * W)[..., ::2], X)),
    "a truth that is not dense": (ALL, lambda who: update(who, 0, X, torch.zeros(2, 4, H, 2 * W)[..., ::2])),
    "clim_index without a climatology": (CLIMS, lambda who: update(who, 0, X, X, K32)),
    "no clim_index, two slots": (CLIMS, lambda who: update(who, 0, X, X, climatology=CLIM2)),
    "an int64 clim_index": (CLIMS, lambda who: update(who, 0, X, X, K32.long(), climatology=CLIM2)),
    "a clim_index of 3 entries": (CLIMS, lambda who: update(who, 0, X, X, torch.zeros(3, dtype=torch.int32),
                                                            climatology=CLIM1)),
    "a climatology of other longitudes": (("Scorecard", "EventTable"),
                                          lambda who: update(who, 0, X, X, climatology=torch.zeros(1, 4, H, W + 2))),
    "other longitudes than bound": (("EventTable", "FractionsTable"),
                                    lambda who: (lambda t: (getattr(t, "bind", lambda w: None)(W),
                                                            t.update(0, torch.zeros(2, 4, H, 6), torch.zeros(2, 4, H, 6))))(new(who))),
}
MESSAGES = {
    ("Scorecard", "names=[]"): "Scorecard: names must list at least one channel",
    ("Spectra", "names=[]"): "Spectra: names must list at least one channel",
    ("EventTable", "names=[]"): "EventTable: names must list at least one channel",
    ("FractionsTable", "names=[]"): "FractionsTable: names must list at least one channel",
    ("Scorecard", "n_leads=0"): "Scorecard: n_leads must be an integer >= 1, got 0",
    ("Spectra", "n_leads=0"): "Spectra: n_leads must be an integer >= 1, got 0",
    ("EventTable", "n_leads=0"): "EventTable: n_leads must be an integer >= 1, got 0",
    ("FractionsTable", "n_leads=0"): "FractionsTable: n_leads must be an integer >= 1, got 0",
    ("Scorecard", "n_leads=True"): "Scorecard: n_leads must be an integer >= 1, got True",
    ("Spectra", "n_leads=True"): "Spectra: n_leads must be an integer >= 1, got True",
    ("EventTable", "n_leads=True"): "EventTable: n_leads must be an integer >= 1, got True",
    ("FractionsTable", "n_leads=True"): "FractionsTable: n_leads must be an integer >= 1, got True",
    ("Spectra", "a latitude of 91"):
        "Spectra: lat_deg must be a vector [H] of finite latitudes in [-90, 90] degrees",
    ("EventTable", "a latitude of 91"):
        "EventTable: lat_deg must be a vector [H] of finite latitudes in [-90, 90] degrees",
    ("FractionsTable", "a latitude of 91"):
        "FractionsTable: lat_deg must be a vector [H] of finite latitudes in [-90, 90] degrees",
    ("Spectra", "weights of the wrong length"): "Spectra: weights must be a floating-point vector [5]",
    ("EventTable", "weights of the wrong length"): "EventTable: weights must be a floating-point vector [5]",
    ("FractionsTable", "weights of the wrong length"): "FractionsTable: weights must be a floating-point vector [5]",
    ("Scorecard", "integer weights"): "Scorecard: lat_weights must be a floating-point vector [H]",
    ("Spectra", "integer weights"): "Spectra: weights must be a floating-point vector [5]",
    ("EventTable", "integer weights"): "EventTable: weights must be a floating-point vector [5]",
    ("FractionsTable", "integer weights"): "FractionsTable: weights must be a floating-point vector [5]",
    ("Scorecard", "negative weights"): "Scorecard: lat_weights must be finite, >= 0 and not all zero",
    ("Spectra", "negative weights"): "Spectra: weights must be finite, >= 0 and not all zero",
    ("EventTable", "negative weights"): "EventTable: weights must be finite, >= 0 and not all zero",
    ("FractionsTable", "negative weights"): "FractionsTable: weights must be finite, >= 0 and not all zero",
    ("Spectra", "bands={}"): "Spectra: bands must be a non-empty dict name -> (lat_lo, lat_hi)",
    ("EventTable", "bands={}"): "EventTable: bands must be a non-empty dict name -> (lat_lo, lat_hi)",
    ("FractionsTable", "bands={}"): "FractionsTable: bands must be a non-empty dict name -> (lat_lo, lat_hi)",
    ("Spectra", "a band that holds no row"): "Spectra: band 'x' (81, 90) holds no row of non-zero weight",
    ("EventTable", "a band that holds no row"): "EventTable: band 'x' (81, 90) holds no row of non-zero weight",
    ("FractionsTable", "a band that holds no row"): "FractionsTable: band 'x' (81, 90) holds no row of non-zero weight",
    ("Spectra", "a band with lo > hi"): "Spectra: band 'x' must have finite lat_lo <= lat_hi, got (10, -10)",
    ("EventTable", "a band with lo > hi"): "EventTable: band 'x' must have finite lat_lo <= lat_hi, got (10, -10)",
    ("FractionsTable", "a band with lo > hi"):
        "FractionsTable: band 'x' must have finite lat_lo <= lat_hi, got (10, -10)",
    ("Spectra", "a band that is no pair"): "Spectra: band 'x' must be (lat_lo, lat_hi) in degrees, got 3",
    ("EventTable", "a band that is no pair"): "EventTable: band 'x' must be (lat_lo, lat_hi) in degrees, got 3",
    ("FractionsTable", "a band that is no pair"): "FractionsTable: band 'x' must be (lat_lo, lat_hi) in degrees, got 3",
    ("Scorecard", "a float64 climatology"): "Scorecard: climatology must be a contiguous float32 [K, 4, 5, W] tensor",
    ("EventTable", "a float64 climatology"): "EventTable: climatology must be a contiguous float32 [K, 4, 5, W] tensor",
    ("FractionsTable", "a float64 climatology"):
        "FractionsTable: climatology must be a contiguous float32 [K, 4, 5, 8] tensor",
    ("Scorecard", "a climatology of 3 channels"):
        "Scorecard: climatology must be a contiguous float32 [K, 4, 5, W] tensor",
    ("EventTable", "a climatology of 3 channels"):
        "EventTable: climatology must be a contiguous float32 [K, 4, 5, W] tensor",
    ("FractionsTable", "a climatology of 3 channels"):
        "FractionsTable: climatology must be a contiguous float32 [K, 4, 5, 8] tensor",
    ("FractionsTable", "n_lon=0"): "FractionsTable: n_lon must be an integer >= 1, got 0",
    ("Scorecard", "lead=True"): "Scorecard.update: lead must be an integer in [0, 2), got True",
    ("Spectra", "lead=True"): "Spectra.update: lead must be an integer in [0, 2), got True",
    ("EventTable", "lead=True"): "EventTable.update: lead must be an integer in [0, 2), got True",
    ("FractionsTable", "lead=True"): "FractionsTable.update: lead must be an integer in [0, 2), got True",
    ("Scorecard", "lead=2"): "Scorecard.update: lead must be an integer in [0, 2), got 2",
    ("Spectra", "lead=2"): "Spectra.update: lead must be an integer in [0, 2), got 2",
    ("EventTable", "lead=2"): "EventTable.update: lead must be an integer in [0, 2), got 2",
    ("FractionsTable", "lead=2"): "FractionsTable.update: lead must be an integer in [0, 2), got 2",
    ("Scorecard", "a 3-d forecast"): "Scorecard.update: forecast must be a [B, C, H, W] tensor",
    ("Spectra", "a 3-d forecast"): "Spectra.update: forecast must be a [B, C, H, W] tensor",
    ("EventTable", "a 3-d forecast"): "EventTable.update: forecast must be a [B, C, H, W] tensor",
    ("FractionsTable", "a 3-d forecast"): "FractionsTable.update: forecast must be a [B, C, H, W] tensor",
    ("Scorecard", "a float64 truth"): "Scorecard.update: truth must be float32, got torch.float64",
    ("Spectra", "a float64 truth"): "Spectra.update: truth must be float32, got torch.float64",
    ("EventTable", "a float64 truth"): "EventTable.update: truth must be float32, got torch.float64",
    ("FractionsTable", "a float64 truth"): "FractionsTable.update: truth must be float32, got torch.float64",
    ("Scorecard", "3 channels"):
        "Scorecard.update: forecast is (2, 3, 5, 8); the scorecard has 4 channels and 5 latitudes",
    ("Spectra", "3 channels"):
        "Spectra.update: forecast is (2, 3, 5, 8); the spectra have 4 channels and 5 latitudes",
    ("EventTable", "3 channels"):
        "EventTable.update: forecast is (2, 3, 5, 8); the table has 4 channels and 5 latitudes",
    ("FractionsTable", "3 channels"):
        "FractionsTable.update: forecast is (2, 3, 5, 8); the table has 4 channels, 5 latitudes and 8 longitudes",
    ("Scorecard", "a truth of another shape"): "Scorecard.update: truth is (1, 4, 5, 8), forecast (2, 4, 5, 8)",
    ("Spectra", "a truth of another shape"): "Spectra.update: truth is (1, 4, 5, 8), forecast (2, 4, 5, 8)",
    ("EventTable", "a truth of another shape"): "EventTable.update: truth is (1, 4, 5, 8), forecast (2, 4, 5, 8)",
    ("FractionsTable", "a truth of another shape"): "FractionsTable.update: truth is (1, 4, 5, 8), forecast (2, 4, 5, 8)",
    ("Scorecard", "a state that is not dense"): "Scorecard.update: forecast must hold dense [C, H, W] states",
    ("Spectra", "a state that is not dense"): "Spectra.update: forecast must hold dense [C, H, W] states",
    ("EventTable", "a state that is not dense"): "EventTable.update: forecast must hold dense [C, H, W] states",
    ("FractionsTable", "a state that is not dense"): "FractionsTable.update: forecast must hold dense [C, H, W] states",
    ("Scorecard", "a truth that is not dense"): "Scorecard.update: truth must hold dense [C, H, W] states",
    ("Spectra", "a truth that is not dense"): "Spectra.update: truth must hold dense [C, H, W] states",
    ("EventTable", "a truth that is not dense"): "EventTable.update: truth must hold dense [C, H, W] states",
    ("FractionsTable", "a truth that is not dense"): "FractionsTable.update: truth must hold dense [C, H, W] states",
    ("Scorecard", "clim_index without a climatology"):
        "Scorecard.update: clim_index given, but the scorecard has no climatology",
    ("EventTable", "clim_index without a climatology"):
        "EventTable.update: clim_index given, but the table has no climatology",
    ("FractionsTable", "clim_index without a climatology"):
        "FractionsTable.update: clim_index given, but the table has no climatology",
    ("Scorecard", "no clim_index, two slots"):
        "Scorecard.update: clim_index is needed to choose among the 2 climatology slots",
    ("EventTable", "no clim_index, two slots"):
        "EventTable.update: clim_index is needed to choose among the 2 climatology slots",
    ("FractionsTable", "no clim_index, two slots"):
        "FractionsTable.update: clim_index is needed to choose among the 2 climatology slots",
    ("Scorecard", "an int64 clim_index"): "Scorecard.update: clim_index must be an int32 tensor [2]",
    ("EventTable", "an int64 clim_index"): "EventTable.update: clim_index must be an int32 tensor [2]",
    ("FractionsTable", "an int64 clim_index"): "FractionsTable.update: clim_index must be an int32 tensor [2]",
    ("Scorecard", "a clim_index of 3 entries"): "Scorecard.update: clim_index must be an int32 tensor [2]",
    ("EventTable", "a clim_index of 3 entries"): "EventTable.update: clim_index must be an int32 tensor [2]",
    ("FractionsTable", "a clim_index of 3 entries"): "FractionsTable.update: clim_index must be an int32 tensor [2]",
    ("Scorecard", "a climatology of other longitudes"): "Scorecard.update: forecast has 8 longitudes, the climatology 10",
    ("EventTable", "a climatology of other longitudes"): "EventTable.update: forecast has 8 longitudes, the climatology 10",
    ("EventTable", "other longitudes than bound"):
        "EventTable.update: forecast has 6 longitudes, the table is bound to 8",
    ("FractionsTable", "other longitudes than bound"):
        "FractionsTable.update: forecast is (2, 4, 5, 6); the table has 4 channels, 5 latitudes and 8 longitudes",
}
ROWS = [(who, what, call) for table in (CONSTRUCTOR, UPDATE) for what, (classes, call) in table.items() for who in classes]


def test_the_table_of_messages_is_complete():
    assert sorted(MESSAGES) == sorted((who, what) for who, what, _ in ROWS)
    assert len(ROWS) >= 80


@pytest.mark.parametrize("who,what,call", ROWS, ids=[f"{who}-{what}" for who, what, _ in ROWS])
def test_refusal_message(who, what, call):
    with pytest.raises(ValueError) as e:
        call(who)
    assert str(e.value) == MESSAGES[(who, what)]


def test_good_arguments_pass_the_checks():
    """the rows above refuse for the reason they name: the good arguments get as far as the device check"""
    for who in GOOD:
        for kw in ({}, {"climatology": CLIM1}, {"climatology": CLIM2}):
            if who == "Spectra" and kw:
                continue
            args = (0, X, X) + ((K32,) if "climatology" in kw and who != "Spectra" else ())
            with pytest.raises(RuntimeError, match="MI355X"):
                update(who, *args, **kw)


# ================================================================================================ Forecaster.run
RUN_KEYS = {"Scorecard": "scorecard", "Spectra": "spectra", "EventTable": "events", "FractionsTable": "fractions"}
RUN_MESSAGES = {
    ("Scorecard", "needs truth"): "Forecaster.run: a scorecard needs truth [B, n_stored, C, H, W] on the device",
    ("Scorecard", "leads"): "Forecaster.run: the scorecard has 1 leads, the rollout stores 2",
    ("Scorecard", "names"):
        "Forecaster.run: the scorecard's names are not the chunk's channel names (PostSpec.names)",
    ("Spectra", "needs truth"): "Forecaster.run: spectra need truth [B, n_stored, C, H, W] on the device",
    ("Spectra", "leads"): "Forecaster.run: the spectra have 1 leads, the rollout stores 2",
    ("Spectra", "names"): "Forecaster.run: the spectra's names are not the chunk's channel names (PostSpec.names)",
    ("EventTable", "needs truth"): "Forecaster.run: an event table needs truth [B, n_stored, C, H, W] on the device",
    ("EventTable", "leads"): "Forecaster.run: the event table has 1 leads, the rollout stores 2",
    ("EventTable", "names"):
        "Forecaster.run: the event table's names are not the chunk's channel names (PostSpec.names)",
    ("FractionsTable", "needs truth"):
        "Forecaster.run: a fractions table needs truth [B, n_stored, C, H, W] on the device",
    ("FractionsTable", "leads"): "Forecaster.run: the fractions table has 1 leads, the rollout stores 2",
    ("FractionsTable", "names"):
        "Forecaster.run: the fractions table's names are not the chunk's channel names (PostSpec.names)",
}


def _forecaster():
    from paradis_model_amd.forecast import Forecaster, PostSpec
    spec = PostSpec.from_features(NAMES[:3], [], zscore_mean=[0.0] * 3, zscore_std=[1.0] * 3, custom_normalization=False,
                                  winds=False, dewpoint=False)
    return Forecaster(None, spec, LAT, np.zeros(W), graph=False)


def _run_table(who, n_leads=2, names=NAMES[:3]):
    return new(who, n_leads=n_leads, names=names, **({"lat_weights": np.ones(H)} if who == "Scorecard" else {}))


@pytest.mark.parametrize("who", list(GOOD))
def test_forecaster_refusals_per_table(who):
    fc = _forecaster()
    inp, forc, const = torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1)
    truth = torch.zeros(1, 2, 3, H, W)
    for what, call in (
            ("needs truth", lambda: fc.run(inp, forc, const, None, truth=None, **{RUN_KEYS[who]: _run_table(who)})),
            ("leads", lambda: fc._check_verification(**{"scorecard": None, RUN_KEYS[who]: _run_table(who, 1)}, truth=truth,
                                                     truth_normalized=False, clim_index=None, B=1, n_stored=2, C=3, H=H, W=W)),
            ("names", lambda: fc._check_verification(**{"scorecard": None, RUN_KEYS[who]: _run_table(who, 2, ["tp", "v10", "u10"])},
                                                     truth=truth, truth_normalized=False, clim_index=None, B=1, n_stored=2,
                                                     C=3, H=H, W=W))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == RUN_MESSAGES[(who, what)], (who, what)


def test_forecaster_refuses_in_the_order_scorecard_spectra_events_fractions():
    """with every table short of leads the scorecard speaks; without it the spectra; and so on"""
    fc = _forecaster()
    truth = torch.zeros(1, 2, 3, H, W)
    tables = {RUN_KEYS[who]: _run_table(who, 1) for who in GOOD}
    for who in GOOD:
        with pytest.raises(ValueError) as e:
            fc._check_verification(**{"scorecard": None, **tables}, truth=truth, truth_normalized=False, clim_index=None,
                                   B=1, n_stored=2, C=3, H=H, W=W)
        assert str(e.value) == RUN_MESSAGES[(who, "leads")]
        with pytest.raises(ValueError) as e:
            fc.run(torch.zeros(1, 1, 6, H, W), torch.zeros(1, 2, H, W, 1), torch.zeros(1, 1, H, W, 1), None, truth=None,
                   **tables)
        assert str(e.value) == RUN_MESSAGES[(who, "needs truth")]
        del tables[RUN_KEYS[who]]


def _member_tables(M):
    from paradis_model_amd.ensemble import EnsembleCard
    from paradis_model_amd.probability import ProbabilityTable
    return {"EnsembleCard": EnsembleCard(NAMES, LAT, 2, M, device="cpu"),
            "ProbabilityTable": ProbabilityTable(NAMES, LAT, 2, EV, M, device="cpu")}


def test_members_is_one_except_for_the_ensemble_tables():
    for who in GOOD:
        assert new(who).members == 1, who
    for who, table in _member_tables(3).items():
        assert table.members == 3, who


def test_table_inputs_are_the_views_run_handed_to_update():
    """``forecast.table_inputs`` against what ``Forecaster.run`` spelt out per table kind: ``t`` and ``k`` for a table of
    single states, ``t[::M]`` (and ``k[::M]``) for an ensemble table, the column only where the table takes one and the
    run has one - the same addresses, shapes and strides, nothing copied"""
    from paradis_model_amd.forecast import table_inputs
    M = 3
    truth = torch.arange(6 * 2 * 3 * 4 * 8, dtype=torch.float32).reshape(6, 2, 3, 4, 8)
    clim_index = torch.arange(12, dtype=torch.int32).reshape(6, 2)
    state = torch.zeros(6, 3, 4, 8)
    view = lambda a: (a.data_ptr(), tuple(a.shape), a.stride(), a.dtype)      # noqa: E731
    same = lambda a, b: view(a) == view(b)                                    # noqa: E731
    tables = {**{who: new(who) for who in GOOD}, **_member_tables(M)}
    for lead in range(2):
        t, k = truth[:, lead], clim_index[:, lead]
        for who, table in tables.items():
            m = M if who in ("EnsembleCard", "ProbabilityTable") else 1
            takes = who not in ("Spectra", "EnsembleCard")
            for col in (k, None):
                got = table_inputs(table, state, t, col)
                assert len(got) == (3 if takes and col is not None else 2), (who, col is None)
                assert got[0] is state
                assert same(got[1], t[::m] if m > 1 else t), who
                assert tuple(got[1].shape) == (6 // m, 3, 4, 8)
                if len(got) == 3:
                    assert same(got[2], k[::m] if m > 1 else k), who
                    assert tuple(got[2].shape) == (6 // m,)
    assert torch.equal(truth, torch.arange(6 * 2 * 3 * 4 * 8, dtype=torch.float32).reshape(6, 2, 3, 4, 8))
