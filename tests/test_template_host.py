"""CPU: the host half of the template path (tf_face_toolbox_amd/verification.py) -- the IJB-style metadata and template-pair
parsers, the CSR grouping, exact TAR@FAR from listed scores, open-set identification, the data-list check -- against
hand-built answers and the float64 restatement (template_ref.py), and the verify.py command line surface."""
import os
import subprocess
import sys

import numpy as np
import pytest

import template_ref as tr
from tf_face_toolbox_amd import verification as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

META = ('TEMPLATE_ID , SUBJECT_ID,FILE,MEDIA_ID,SIGHTING_ID,FACE_X,score\n'
        '7,70,img/1.jpg,100,1,3.5,0.5\n'
        '3,30,frame/10_1.png,200,2,1,1.0\n'
        '7,70,frame/11_1.png,300,3,0,2.0\n'
        '3,30,frame/10_2.png,200,4,0,0.0\n'
        '7,70,img/2.jpg,100,5,0,1.5\n'
        '3,30,img/1.jpg,400,6,0,1.0\n'
        '9,31,img/9.jpg,900,7,0,1.0\n')


def _meta(tmp_path, text=META, weight=None):
    p = tmp_path / 'meta.csv'
    p.write_text(text)
    return V.read_template_metadata(str(p), weight)


def test_metadata_parser_reads_columns_by_name(tmp_path):
    m = _meta(tmp_path, weight='score')
    assert m['template'].tolist() == [7, 3, 7, 3, 7, 3, 9]
    assert m['subject'].tolist() == [70, 30, 70, 30, 70, 30, 31]
    assert m['file'][1] == 'frame/10_1.png' and m['media'][1] == '200'
    assert np.allclose(m['weight'], [0.5, 1.0, 2.0, 0.0, 1.5, 1.0, 1.0])
    assert _meta(tmp_path)['weight'] is None
    # column order does not matter, extra columns are ignored
    text = 'FACE_Y,MEDIA_ID,FILE,TEMPLATE_ID,SUBJECT_ID\n1,5,a.jpg,2,20\n2,6,b.jpg,2,20\n'
    m = _meta(tmp_path, text)
    assert m['template'].tolist() == [2, 2] and m['media'] == ['5', '6'] and m['file'] == ['a.jpg', 'b.jpg']
    with pytest.raises(ValueError, match='MEDIA_ID'):
        _meta(tmp_path, 'TEMPLATE_ID,SUBJECT_ID,FILE\n1,2,a.jpg\n')
    with pytest.raises(ValueError, match='no column'):
        _meta(tmp_path, weight='quality')


def test_metadata_refuses_a_template_with_two_subjects(tmp_path):
    with pytest.raises(ValueError, match='template 4 names subjects 1 and 2'):
        _meta(tmp_path, 'TEMPLATE_ID,SUBJECT_ID,FILE,MEDIA_ID\n4,1,a.jpg,1\n4,2,b.jpg,2\n')


def test_build_templates(tmp_path):
    t = V.build_templates(_meta(tmp_path))
    assert t['template_ids'].tolist() == [3, 7, 9] and t['subjects'].tolist() == [30, 70, 31]
    # template 3: media 200 (rows 1, 3), media 400 (row 5); template 7: media 100 (rows 0, 4), 300 (row 2); template 9: row 6
    assert t['members'].tolist() == [1, 3, 5, 0, 4, 2, 6]
    assert t['media_off'].tolist() == [0, 2, 3, 5, 6, 7]
    assert t['tmpl_off'].tolist() == [0, 2, 4, 5]
    assert t['members'].dtype == np.int32 and t['tmpl_off'].dtype == np.int32
    assert V.template_sizes(t['media_off'], t['tmpl_off']).tolist() == [3, 3, 1]
    assert V.template_index(t['template_ids'], [9, 3]).tolist() == [2, 0]
    with pytest.raises(KeyError, match='template 5'):
        V.template_index(t['template_ids'], [3, 5])


def test_pooling_restatement_hand_built():
    x = np.array([[1.0, 0.0], [0.0, 1.0], [3.0, 4.0], [5.0, 5.0]])
    # template 0: media {0, 1} with weights 1, 3 -> (0.25, 0.75), plus media {2} -> (3, 4); template 1: media {3} of weight 0
    got = tr.pool(x, [0, 1, 2, 3], [0, 2, 3, 4], [0, 2, 3, 3], w=[1.0, 3.0, 2.0, 0.0])
    v = np.array([0.25 + 3.0, 0.75 + 4.0])
    assert np.allclose(got[0], v / np.linalg.norm(v))
    assert np.all(got[1] == 0)                      # a zero-weight media only: nothing
    assert np.all(got[2] == 0)                      # no media


def test_template_pairs_parser(tmp_path):
    p = tmp_path / 'pairs.csv'
    p.write_text('ENROLL_TEMPLATE_ID,VERIF_TEMPLATE_ID\n3,7\n7,9\n3,3\n')
    t1, t2, g = V.read_template_pairs(str(p), {3: 30, 7: 70, 9: 70})
    assert t1.tolist() == [3, 7, 3] and t2.tolist() == [7, 9, 3] and g.tolist() == [False, True, True]
    p.write_text('3 7 1\n7 9 0\n\n9 3 1\n')
    t1, t2, g = V.read_template_pairs(str(p))
    assert t1.tolist() == [3, 7, 9] and g.tolist() == [True, False, True]
    p.write_text('3,7\n')
    with pytest.raises(ValueError, match='no label'):
        V.read_template_pairs(str(p))
    with pytest.raises(ValueError, match='template 7'):
        V.read_template_pairs(str(p), {3: 1})


def test_tar_at_far_exact_with_ties_and_na():
    # 10 impostors with ties, 4 genuine
    imp = [0.9, 0.8, 0.8, 0.7, 0.5, 0.5, 0.5, 0.2, 0.1, 0.0]
    gen = [0.95, 0.8, 0.6, 0.5]
    scores = np.array(gen + imp)
    genuine = np.array([True] * 4 + [False] * 10)
    rows = V.tar_at_far_scores(scores, genuine, fars=(0.1, 0.2, 0.5, 0.01))
    # FAR 0.1: k = 1 -> i_1 = 0.8, accept s > 0.8: genuine {0.95} -> 0.25, impostors {0.9} -> 0.1
    assert rows[0]['threshold'] == 0.8 and rows[0]['tar'] == 0.25 and rows[0]['achieved_far'] == 0.1
    # FAR 0.2: k = 2 -> i_2 = 0.8 (tie): still s > 0.8
    assert rows[1]['threshold'] == 0.8 and rows[1]['tar'] == 0.25 and rows[1]['achieved_far'] == 0.1
    # FAR 0.5: k = 5 -> i_5 = 0.5, accept s > 0.5: genuine 3/4, impostors 4/10
    assert rows[2]['threshold'] == 0.5 and rows[2]['tar'] == 0.75 and rows[2]['achieved_far'] == 0.4
    assert rows[3]['tar'] == 'n/a'                  # 10 impostors < 1 / 0.01
    ref = tr.tar_at_far(scores, genuine, (0.1, 0.2, 0.5, 0.01))
    for row, r in zip(rows, ref):
        assert (r is None) == (row['tar'] == 'n/a')
        if r is not None:
            assert (row['tar'], row['achieved_far'], row['threshold']) == r
    rng = np.random.default_rng(3)
    s = np.round(rng.standard_normal(5000), 2)      # many ties
    g = rng.random(5000) < 0.2
    fars = (1e-4, 1e-3, 1e-2, 1e-1)
    for row, r in zip(V.tar_at_far_scores(s, g, fars), tr.tar_at_far(s, g, fars)):
        assert (r is None) == (row['tar'] == 'n/a')
        if r is not None:
            assert abs(row['tar'] - r[0]) < 1e-12 and abs(row['achieved_far'] - r[1]) < 1e-12 and row['threshold'] == r[2]
            assert row['achieved_far'] <= row['far']
    with pytest.raises(ValueError, match='NaN'):
        V.tar_at_far_scores([np.nan, 0.1], [True, False])


def test_open_set_identification_hand_built():
    gallery_subjects = [10, 20, 30]
    # probes: subject 10 (mated, mate first), 20 (mated, mate second), 40 (non-mated), 50 (non-mated), 30 (mated, mate first)
    probe_subjects = [10, 20, 40, 50, 30]
    S = np.array([[0.9, 0.1, 0.0],
                  [0.7, 0.6, 0.1],
                  [0.5, 0.2, 0.1],
                  [0.3, 0.8, 0.2],
                  [0.1, 0.2, 0.4]])
    idx = np.argsort(-S, 1, kind='stable')
    sc = np.take_along_axis(S, idx, 1)
    r = V.open_set_identification(sc, idx, probe_subjects, gallery_subjects, ranks=(1, 2, 3), fpirs=(0.5, 0.1))
    assert r['mated'] == 3 and r['non_mated'] == 2
    assert r['cmc'] == {1: 2 / 3.0, 2: 1.0, 3: 1.0}
    # FPIR 0.5: non-mated top-1 scores {0.5, 0.8}, k = 1 -> threshold 0.5: mated rank-1 hits above it: 0.9 only (0.4 is not)
    t = r['tpir_at_fpir'][0]
    assert t['threshold'] == 0.5 and t['tpir'] == 1 / 3.0 and t['achieved_fpir'] == 0.5
    assert r['tpir_at_fpir'][1]['tpir'] == 'n/a'     # 2 non-mated probes < 1 / 0.1
    cmc, tp = tr.open_set(S, probe_subjects, gallery_subjects, (1, 2, 3), (0.5, 0.1))
    assert cmc == r['cmc'] and tp == [1 / 3.0, None]


def test_data_list_check_and_template_list(tmp_path):
    m = _meta(tmp_path)
    out = tmp_path / 'list.txt'
    V.write_template_list(m, '/data/ijba', str(out))
    from tf_face_toolbox_amd.data import get_image_paths
    paths, n = get_image_paths(str(out))
    assert n == 7 and paths[0] == '/data/ijba/img/1.jpg' and paths[1] == '/data/ijba/frame/10_1.png'
    assert out.read_text().splitlines()[1].split()[1] == '30'
    V.check_data_list(paths, m)
    with pytest.raises(ValueError, match='6 images, the template metadata has 7'):
        V.check_data_list(paths[:6], m)
    bad = list(paths)
    bad[3] = '/data/ijba/frame/10_3.png'
    with pytest.raises(ValueError, match='row 3 is /data/ijba/frame/10_3.png, but metadata row 3 names FILE frame/10_2.png'):
        V.check_data_list(bad, m)
    bad = list(paths)
    bad[0] = '/data/ijba/ximg/1.jpg'                 # a suffix, but not at a path-component boundary
    with pytest.raises(ValueError, match='row 0'):
        V.check_data_list(bad, m)


def test_verify_cli_template_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'verify.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ('templates', 'template_search', '--template_metadata', '--template_pairs', '--fusion', '--betas',
                '--gallery_metadata', '--splits', '--weight_column'):
        assert opt in r.stdout, opt
    sys.path.insert(0, ROOT)
    import verify
    assert verify.parse_betas('0:20') == list(range(21))
    assert verify.parse_betas('0:40:10') == [0, 10, 20, 30, 40]
    assert verify.parse_betas('1,2.5') == [1.0, 2.5]
    assert verify.parse_splits('1-10') == [str(i) for i in range(1, 11)]
    assert verify.parse_splits('2,5') == ['2', '5'] and verify.parse_splits(None) == [None]
    s = verify.summarise_splits([{'tar_at_far': [{'far': 0.1, 'tar': 0.5}], 'cmc': {'1': 0.2}},
                                 {'tar_at_far': [{'far': 0.1, 'tar': 0.7}], 'cmc': {'1': 0.4}}])
    assert abs(s['TAR@FAR=0.1']['mean'] - 0.6) < 1e-12 and abs(s['TAR@FAR=0.1']['std'] - 0.1) < 1e-12
    assert abs(s['rank-1']['mean'] - 0.3) < 1e-12
