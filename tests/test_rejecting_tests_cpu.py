"""CPU: the table of the tests that can reject a detection (semisup_infer.TESTS), entry by entry on arrays written by hand, and that
autolabel counts the same rows as rejected when it is given them as records.  Booleans and integers are compared: no tolerance."""
import numpy as np

from transferable3d_amd import autolabel as AL, floor as FL, semisup_infer as SI, visibility as VS

NAN = float('nan')
LOW = [0.5, np.nextafter(0.5, 0.0), NAN, 0.75]                 # against a lower limit of 0.5: at it, just below it, a NaN, above it
LOW_REJECTED = [False, True, True, False]
# flag -> (limit, parameters, {field: column}, the rows the test rejects)
CASES = {
    'min_reproj_iou': (0.5, {}, {'reproj_iou': LOW}, LOW_REJECTED),
    'min_mask_in_box': (0.5, {}, {'mask_in_box': LOW}, LOW_REJECTED),
    'min_seg_box_iou': (0.5, {}, {'seg_box_iou': LOW}, LOW_REJECTED),
    'min_view_iou': (0.5, {}, {'view_iou': LOW}, LOW_REJECTED),
    'min_rescore': (0.5, {}, {'rescore_prob': LOW}, LOW_REJECTED),
    # at the limit, just beyond it, a NaN, sunk beyond it, sunk to it, and far beyond it with each flag of floor.UNKNOWN
    'max_floor_gap': (0.25, {}, {'floor_gap': [0.25, np.nextafter(0.25, 1.0), NAN, -0.5, -0.25, 0.75, NAN, 0.75],
                                 'floor_flags': [0, 0, 0, 0, FL.TOO_FAR, FL.NO_FLOOR, FL.NOT_FINITE, FL.NO_FLOOR | FL.NOT_FINITE]},
                      [False, True, False, True, False, False, False, False]),
    # at the limit, just beyond it, a NaN, far beyond it with each flag of visibility.UNMEASURED, on min_rays - 1 rays, on min_rays rays,
    # and with a flag outside UNMEASURED
    'max_see_through': (0.5, {'min_rays': 8}, {'see_through': [0.5, np.nextafter(0.5, 1.0), NAN, 0.75, 0.75, 0.75, 0.75, 0.75, 0.75],
                                               'visibility_evidence': [20, 20, 20, 20, 20, 20, 7, 8, 20],
                                               'visibility_flags': [0, 0, 0, VS.NO_SCENE, VS.NOT_FINITE, VS.BEHIND, 0, 0, VS.NO_EVIDENCE]},
                        [False, True, False, False, False, False, False, True, True]),
}


def test_the_table_names_every_test_once_and_in_the_order_of_the_log_line():
    assert [t.flag for t in SI.TESTS] == list(CASES)
    assert [t.fragment for t in SI.TESTS] == ['reproj_iou < %g', 'mask_in_box < %g', 'seg_box_iou < %g', 'view_iou < %g', 'rescore_prob < %g',
                                              '|floor_gap| > %g', 'see_through > %g']
    assert VS.UNMEASURED == VS.NO_SCENE | VS.NOT_FINITE | VS.BEHIND and FL.UNKNOWN == FL.NO_FLOOR | FL.NOT_FINITE
    assert VS.evidence(np.array([[9, 1, 2, 3, 4, 5]])).tolist() == [3 + 4]          # inside + through of a profile row


def test_every_entry_rejects_the_rows_written_out_and_autolabel_counts_the_same():
    for test in SI.TESTS:
        limit, parameters, columns, want = CASES[test.flag]
        assert tuple(columns) == test.fields and tuple(parameters) == test.parameters, test.flag
        got = test.rejected(*(np.array(columns[k]) for k in test.fields), limit, **parameters)
        assert got.dtype == bool and got.tolist() == want, (test.flag, got.tolist())
        records = [dict({'class': 'chair', 'detected': True, 'accepted': True}, **{k: v[i] for k, v in columns.items()}) for i in range(len(want))]
        records.insert(1, {'class': 'chair', 'detected': False, 'accepted': False})          # too few points: no test sees it
        active = [(test, limit, parameters)]
        rows = [r for r in records if r['detected']]
        assert AL.rejected_by(active, rows)[test.flag].tolist() == want, test.flag
        c = AL.count(records, ['chair', 'sofa'], active)
        assert c['chair']['rejected_by'] == {test.flag: sum(want)} and c['chair']['offered'] == len(want) + 1 and c['chair']['too_few_points'] == 1
        assert c['sofa']['rejected_by'] == {test.flag: 0} and type(c['chair']['rejected_by'][test.flag]) is int


def test_active_tests_reads_the_limits_under_the_flags_names():
    floor, visibility = FL.check_options(max_floor_gap=0.25), VS.check_options(max_see_through=0.5, visibility_min_rays=8)
    assert SI.active_tests(None, FL.check_options(floor=True), VS.check_options(visibility=True)) == []
    active = SI.active_tests(None, visibility, floor)                  # the order is the table's, not the holders'
    assert [(t.flag, limit, p) for t, limit, p in active] == [('max_floor_gap', 0.25, {}), ('max_see_through', 0.5, {'min_rays': 8})]
