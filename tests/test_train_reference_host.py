"""CPU: the float64 training reference oracle/prednet_train_ref.py, pinned.  It is the only statement that the HIP gradients are
right (tests/test_gpu_train*.py compare the trainer against it), so its own values are recorded here.

The literals were recorded on the CPU from the three per-file restatements this module replaced (`_ref`, `_ref_ext`, `_ref_obj` of
tests/test_gpu_train*.py) at (w, h, channels) = (16, 12, [3, 4, 6]), synthetic weights seed 1, _drifting(19, 2, 6, 3, 12, 16),
n_fed = 3, float feedback, step weights [0, 1, 0.5, 2, 1.5], L_all = [1, 0.1, 0.1]; the plain values are the teacher-forced,
unweighted squared error.  No gradient norm is zero at this shape under any of the three settings.

Bound: 1e-12 relative.  Two orders of the same float64 sums (one sum over all terms against the mean of per-step means) were
measured 2e-16 apart; 1e-12 leaves four orders for another torch build and is seven orders below the tightest bound a GPU test
puts on the trainer (1e-5)."""
import numpy as np

from evolutionary_illusion_generator_amd import train, weights
from oracle import prednet_train_ref as ref
from tests.train_support import _drifting

W, H, CH = 16, 12, [3, 4, 6]
N_FED, STEP_W, LALL = 3, [0.0, 1.0, 0.5, 2.0, 1.5], [1.0, 0.1, 0.1]
TOL = 1e-12

PLAIN_LOSS = 0.004989665116457212
MSE_LOSS = 0.01928674504653576
LALL_LOSS = 0.05235199028402857
STEP_MSE = [0.006647834043953292, 0.004203307209487775, 0.00450652188533255, 0.017563266175797416, 0.036567083152619945]
TABLE = [[0.033619893814433796, 0.017153100630821903, 0.008728551203763396],
         [0.025932158535358532, 0.0074236025994331946, 0.0029573572512933658],
         [0.026632465317376397, 0.001415859091957454, 0.0005408872639637897],
         [0.052990739072433235, 0.0007078113046778079, 0.00029549891395014137],
         [0.07674554261254068, 0.0003377939648269148, 0.00016335814066861527]]
# Frobenius norm of every gradient tensor
PLAIN_NORMS = {
    'ConvP0/W': 0.014388947910130328, 'ConvP0/b': 0.007753415229050747, 'ConvLSTM0/x_i0/W': 0.00045592194757372096,
    'ConvLSTM0/x_i1/W': 1.4531730770082212e-05, 'ConvLSTM0/h_i/W': 0.00022330150935872734, 'ConvLSTM0/h_i/b': 0.00018637123964471435,
    'ConvLSTM0/x_f0/W': 8.181951567337256e-05, 'ConvLSTM0/x_f1/W': 1.1684045495425175e-05, 'ConvLSTM0/h_f/W': 0.0004552835860534897,
    'ConvLSTM0/h_f/b': 0.0001853836370946004, 'ConvLSTM0/x_c0/W': 0.018047026393083317, 'ConvLSTM0/x_c1/W': 0.0011657980723273331,
    'ConvLSTM0/h_c/W': 0.0390133403264538, 'ConvLSTM0/h_c/b': 0.014532775191054921, 'ConvLSTM0/x_o0/W': 0.00030601895332628366,
    'ConvLSTM0/x_o1/W': 9.04273283827855e-06, 'ConvLSTM0/h_o/W': 0.00013519080595170138, 'ConvLSTM0/h_o/b': 8.802621281385692e-05,
    'ConvLSTM0/c_i/W': 4.897086993174133e-06, 'ConvLSTM0/c_f/W': 1.80592306605114e-05, 'ConvLSTM0/c_o/W': 4.967768709799342e-06,
    'ConvA1/W': 9.845760708579645e-05, 'ConvA1/b': 0.00013423839453750543, 'ConvP1/W': 6.2495066634660835e-06, 'ConvP1/b': 9.555943841672377e-05,
    'ConvLSTM1/x_i0/W': 5.235183193502935e-06, 'ConvLSTM1/x_i1/W': 1.6465046978028706e-07, 'ConvLSTM1/h_i/W': 4.3561048294625245e-07,
    'ConvLSTM1/h_i/b': 9.13963946021555e-06, 'ConvLSTM1/x_f0/W': 1.060884153032146e-06, 'ConvLSTM1/x_f1/W': 9.815758234474101e-08,
    'ConvLSTM1/h_f/W': 4.533972210692017e-07, 'ConvLSTM1/h_f/b': 5.507963546838979e-06, 'ConvLSTM1/x_c0/W': 0.00020683446527094203,
    'ConvLSTM1/x_c1/W': 1.1154977620301094e-05, 'ConvLSTM1/h_c/W': 4.220049298687098e-05, 'ConvLSTM1/h_c/b': 0.000670930243541623,
    'ConvLSTM1/x_o0/W': 4.554064374875227e-06, 'ConvLSTM1/x_o1/W': 1.540696906721749e-07, 'ConvLSTM1/h_o/W': 5.381789320001941e-07,
    'ConvLSTM1/h_o/b': 9.017816709215133e-06, 'ConvLSTM1/c_i/W': 7.682366609076423e-08, 'ConvLSTM1/c_f/W': 1.1017416414037748e-07,
    'ConvLSTM1/c_o/W': 1.0836511855414745e-07, 'ConvA2/W': 1.0220728593096905e-05, 'ConvA2/b': 3.0551321549173206e-05,
    'ConvP2/W': 3.9965351741438324e-07, 'ConvP2/b': 1.715893844304832e-05, 'ConvLSTM2/x_i0/W': 4.524930372178469e-08,
    'ConvLSTM2/h_i/W': 3.8379597250342306e-09, 'ConvLSTM2/h_i/b': 3.769238431912503e-07, 'ConvLSTM2/x_f0/W': 1.6879199387851145e-08,
    'ConvLSTM2/h_f/W': 4.372476875652287e-09, 'ConvLSTM2/h_f/b': 2.450002160445547e-07, 'ConvLSTM2/x_c0/W': 1.0835323408879445e-05,
    'ConvLSTM2/h_c/W': 1.655907689546492e-06, 'ConvLSTM2/h_c/b': 0.0001252028470143226, 'ConvLSTM2/x_o0/W': 3.309216391598005e-08,
    'ConvLSTM2/h_o/W': 5.292514150004938e-09, 'ConvLSTM2/h_o/b': 3.7651904564761594e-07, 'ConvLSTM2/c_i/W': 1.2086032358114983e-09,
    'ConvLSTM2/c_f/W': 1.488178266457422e-09, 'ConvLSTM2/c_o/W': 1.749959352989014e-09}
MSE_NORMS = {
    'ConvP0/W': 0.02539549326471645, 'ConvP0/b': 0.006167181926008577, 'ConvLSTM0/x_i0/W': 0.00010537583197573786,
    'ConvLSTM0/x_i1/W': 7.637582305176435e-06, 'ConvLSTM0/h_i/W': 0.00027000945539308965, 'ConvLSTM0/h_i/b': 0.0001335841999441175,
    'ConvLSTM0/x_f0/W': 0.00018617332026092128, 'ConvLSTM0/x_f1/W': 4.6014450793370674e-05, 'ConvLSTM0/h_f/W': 0.002356482341593788,
    'ConvLSTM0/h_f/b': 0.0009625284739597794, 'ConvLSTM0/x_c0/W': 0.01859047834734365, 'ConvLSTM0/x_c1/W': 0.0035548349649854884,
    'ConvLSTM0/h_c/W': 0.2074187504420221, 'ConvLSTM0/h_c/b': 0.0767743480854685, 'ConvLSTM0/x_o0/W': 0.00037765412608275865,
    'ConvLSTM0/x_o1/W': 3.004295753832751e-05, 'ConvLSTM0/h_o/W': 0.00028633549932430833, 'ConvLSTM0/h_o/b': 7.753083549090706e-05,
    'ConvLSTM0/c_i/W': 1.0998353423436403e-05, 'ConvLSTM0/c_f/W': 9.691017992342611e-05, 'ConvLSTM0/c_o/W': 1.7577463545526624e-05,
    'ConvA1/W': 0.0002601999130254832, 'ConvA1/b': 0.0004302280589087945, 'ConvP1/W': 2.5750345436492123e-05, 'ConvP1/b': 0.00030985490406644105,
    'ConvLSTM1/x_i0/W': 9.626010655351893e-06, 'ConvLSTM1/x_i1/W': 4.897469143672833e-07, 'ConvLSTM1/h_i/W': 1.743648047413013e-06,
    'ConvLSTM1/h_i/b': 2.392804709969886e-05, 'ConvLSTM1/x_f0/W': 3.6812466854536745e-06, 'ConvLSTM1/x_f1/W': 4.52615909629182e-07,
    'ConvLSTM1/h_f/W': 2.2210551416718873e-06, 'ConvLSTM1/h_f/b': 2.7432582404754656e-05, 'ConvLSTM1/x_c0/W': 0.0006052092118581237,
    'ConvLSTM1/x_c1/W': 5.245039841710345e-05, 'ConvLSTM1/h_c/W': 0.0002172270465481443, 'ConvLSTM1/h_c/b': 0.003498641115369503,
    'ConvLSTM1/x_o0/W': 3.6664933816781464e-06, 'ConvLSTM1/x_o1/W': 3.7008765951249366e-07, 'ConvLSTM1/h_o/W': 1.958508152656754e-06,
    'ConvLSTM1/h_o/b': 2.3786220271834175e-05, 'ConvLSTM1/c_i/W': 2.971863635999446e-07, 'ConvLSTM1/c_f/W': 6.601380115540963e-07,
    'ConvLSTM1/c_o/W': 4.108843423346149e-07, 'ConvA2/W': 4.9789332059498124e-05, 'ConvA2/b': 0.00016807371696600791,
    'ConvP2/W': 2.4639573219137056e-06, 'ConvP2/b': 0.00011270034998481092, 'ConvLSTM2/x_i0/W': 2.1092402562741988e-07,
    'ConvLSTM2/h_i/W': 1.831394098220648e-08, 'ConvLSTM2/h_i/b': 1.6767216704673858e-06, 'ConvLSTM2/x_f0/W': 7.759913635939189e-08,
    'ConvLSTM2/h_f/W': 2.4698859023975264e-08, 'ConvLSTM2/h_f/b': 1.338581676235422e-06, 'ConvLSTM2/x_c0/W': 5.451140586943596e-05,
    'ConvLSTM2/h_c/W': 9.778112293330554e-06, 'ConvLSTM2/h_c/b': 0.0007358795102403485, 'ConvLSTM2/x_o0/W': 1.2789975010301066e-07,
    'ConvLSTM2/h_o/W': 2.574150608919044e-08, 'ConvLSTM2/h_o/b': 1.6755352057704173e-06, 'ConvLSTM2/c_i/W': 6.350522670927039e-09,
    'ConvLSTM2/c_f/W': 9.044243126653608e-09, 'ConvLSTM2/c_o/W': 9.728909983617703e-09}
LALL_NORMS = {
    'ConvP0/W': 0.03189993149298072, 'ConvP0/b': 0.006680500194676624, 'ConvLSTM0/x_i0/W': 0.0002049423992207429,
    'ConvLSTM0/x_i1/W': 1.1772745788944158e-05, 'ConvLSTM0/h_i/W': 0.0004885247774010453, 'ConvLSTM0/h_i/b': 0.00022499628028295368,
    'ConvLSTM0/x_f0/W': 0.0002420592035448516, 'ConvLSTM0/x_f1/W': 5.818685776196005e-05, 'ConvLSTM0/h_f/W': 0.0026723497812542623,
    'ConvLSTM0/h_f/b': 0.0010798231439040592, 'ConvLSTM0/x_c0/W': 0.025224170452930496, 'ConvLSTM0/x_c1/W': 0.004972569881905507,
    'ConvLSTM0/h_c/W': 0.24982451060776112, 'ConvLSTM0/h_c/b': 0.09083433387235121, 'ConvLSTM0/x_o0/W': 0.0005816209752406589,
    'ConvLSTM0/x_o1/W': 3.774575540579112e-05, 'ConvLSTM0/h_o/W': 0.00034919577428875866, 'ConvLSTM0/h_o/b': 0.0001271975791026914,
    'ConvLSTM0/c_i/W': 1.7892969791886405e-05, 'ConvLSTM0/c_f/W': 0.00013554363177804176, 'ConvLSTM0/c_o/W': 3.071706505996901e-05,
    'ConvA1/W': 0.0008272213537430955, 'ConvA1/b': 0.003706748924591893, 'ConvP1/W': 0.0003110221708407832, 'ConvP1/b': 0.014022419105334343,
    'ConvLSTM1/x_i0/W': 9.594220820948529e-06, 'ConvLSTM1/x_i1/W': 4.736309675645417e-07, 'ConvLSTM1/h_i/W': 1.9904865548411177e-06,
    'ConvLSTM1/h_i/b': 2.5653017829309504e-05, 'ConvLSTM1/x_f0/W': 3.129272091577686e-06, 'ConvLSTM1/x_f1/W': 4.02109988688734e-07,
    'ConvLSTM1/h_f/W': 2.252462853748311e-06, 'ConvLSTM1/h_f/b': 3.333961481839642e-05, 'ConvLSTM1/x_c0/W': 0.0006806694553835377,
    'ConvLSTM1/x_c1/W': 6.773257390509395e-05, 'ConvLSTM1/h_c/W': 0.0003160380076974469, 'ConvLSTM1/h_c/b': 0.005616310674113355,
    'ConvLSTM1/x_o0/W': 5.276890248630559e-06, 'ConvLSTM1/x_o1/W': 3.9748255875110837e-07, 'ConvLSTM1/h_o/W': 1.995225156938303e-06,
    'ConvLSTM1/h_o/b': 2.5658562578188543e-05, 'ConvLSTM1/c_i/W': 3.6434373395487473e-07, 'ConvLSTM1/c_f/W': 8.470462318322327e-07,
    'ConvLSTM1/c_o/W': 5.302528372723408e-07, 'ConvA2/W': 0.0004521135166595585, 'ConvA2/b': 0.012160262971620647, 'ConvP2/W': 7.127918888473909e-05,
    'ConvP2/b': 0.01028133715928891, 'ConvLSTM2/x_i0/W': 5.50294798988898e-07, 'ConvLSTM2/h_i/W': 6.249336771400578e-08,
    'ConvLSTM2/h_i/b': 5.352337001120466e-06, 'ConvLSTM2/x_f0/W': 2.546843107781496e-07, 'ConvLSTM2/h_f/W': 1.1078176197645455e-07,
    'ConvLSTM2/h_f/b': 6.796925944272463e-06, 'ConvLSTM2/x_c0/W': 0.00013821467525331523, 'ConvLSTM2/h_c/W': 3.1913859459430786e-05,
    'ConvLSTM2/h_c/b': 0.0025975696727147477, 'ConvLSTM2/x_o0/W': 2.185759878409789e-07, 'ConvLSTM2/h_o/W': 7.257422057970947e-08,
    'ConvLSTM2/h_o/b': 5.346324381707549e-06, 'ConvLSTM2/c_i/W': 1.741111400591904e-08, 'ConvLSTM2/c_f/W': 3.7583737170377984e-08,
    'ConvLSTM2/c_o/W': 2.1996066104923564e-08}


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= TOL * np.abs(want)).all())


def _norms_match(grads, want):
    assert sorted(grads) == sorted(want)
    for k, n in want.items():
        assert n > 0.0, k
        assert _close(np.linalg.norm(grads[k].ravel()), n), (k, np.linalg.norm(grads[k].ravel()), n)


def test_the_reference_reproduces_its_recorded_values():
    wts = weights.synthetic_prednet_weights(CH, W, H, seed=1)
    frames = _drifting(19, 2, 6, 3, 12, 16)
    plain = ref.run(wts, CH, frames)
    assert _close(plain.loss, PLAIN_LOSS), (plain.loss, PLAIN_LOSS)
    _norms_match(plain.grads, PLAIN_NORMS)

    mse = ref.run(wts, CH, frames, n_fed=N_FED, requant=False, step_weights=STEP_W)
    assert _close(mse.loss, MSE_LOSS), (mse.loss, MSE_LOSS)
    assert _close(mse.step_mse, STEP_MSE), (mse.step_mse, STEP_MSE)
    assert _close(mse.table, TABLE), (mse.table, TABLE)
    _norms_match(mse.grads, MSE_NORMS)

    err = ref.run(wts, CH, frames, objective="error", layer_weights=LALL, n_fed=N_FED, requant=False, step_weights=STEP_W)
    assert _close(err.loss, LALL_LOSS), (err.loss, LALL_LOSS)
    assert _close(err.step_mse, STEP_MSE) and _close(err.table, TABLE)
    assert np.array_equal(err.pred, mse.pred)
    _norms_match(err.grads, LALL_NORMS)
    want = train.combine_terms(err.table, LALL, STEP_W)
    assert abs(err.loss - want) <= TOL * want, (err.loss, want)
    # and the weighted squared error is the stated combination of the per-step values
    want = sum(w * m for w, m in zip(STEP_W, mse.step_mse)) / sum(STEP_W)
    assert abs(mse.loss - want) <= TOL * want, (mse.loss, want)


def test_one_frame_has_no_term_and_the_state_continues_a_sequence():
    wts = weights.synthetic_prednet_weights(CH, W, H, seed=1)
    frames = _drifting(19, 2, 6, 3, 12, 16)
    for objective in ("mse", "error"):
        one = ref.run(wts, CH, frames[:, :1], objective=objective)
        assert one.loss == 0.0 and one.table.shape == (0, 3) and one.step_mse.shape == (0,)
        assert all(not np.any(g) for g in one.grads.values())
    # two pieces give the predictions of one call: the state carries everything a later step reads
    whole = ref.run(wts, CH, frames)
    first = ref.run(wts, CH, frames[:, :2])
    second = ref.run(wts, CH, frames[:, 2:], state=first.state)
    assert np.array_equal(np.concatenate([first.pred, second.pred], 1), whole.pred)
    assert np.array_equal(second.step_mse, whole.step_mse[2:]) and np.array_equal(second.table, whole.table[2:])
